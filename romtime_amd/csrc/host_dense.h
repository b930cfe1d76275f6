// Host-side small dense helpers of libromtime_hip.so (plain C++: also built with g++ and sanitizers by the CPU tests).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/romtime_hip.h"

// ---- the decisions rt_pod_orth takes from a spectrum -------------------------------------------------------------------------
// Stated once here for the C side; romtime_amd/pod_rules.py states them once for the Python side, and
// tests/test_pod_rules_cpu.py runs both on the same spectra (through tests/host/host_dense_check.cpp).
constexpr double RT_DROP_TOLERANCE = 1e-7;  // pod.py:4 (the docstring says 1e-8; the code is 1e-7)
constexpr double RT_TWO_PASS_RATIO = 1e-2;  // one Gram pass resolves vectors to eps (sigma_1/sigma_i)^2
constexpr double RT_RR_GAP = 1e-4;          // eigenvalue gap (relative to lambda_1) below which inverse iteration is not trusted
constexpr double RT_LEVEL_RATIO = 0.08;     // a deflated level accepts the modes within this ratio of its largest (pod_rules.py)
constexpr int RT_MAX_LEVELS = 16;

// sigma_i = sqrt(max(lam_i, 0))
std::vector<double> rt_sigma(const std::vector<double>& lam);

// energy_i = (s_0^2 + ... + s_i^2) / total   (NaN for an all-zero matrix, as the reference)
void rt_energy(const std::vector<double>& s, double total, std::vector<double>& energy);

// Number of modes `orth` keeps: tol != 0 -> energy < tol (strict); else num != 0 -> min(num, n); else sigma > 1e-7.
int rt_truncation_rank(const std::vector<double>& s, const std::vector<double>& energy, int64_t num, double tol);

// Every gap among the k largest eigenvalues, and to the next one (to zero when k == n), is at least RR_GAP lam_1: the
// inverse-iteration vectors are used as they are, otherwise they get a k x k Rayleigh-Ritz step.
bool rt_separated(const std::vector<double>& lam, int k);

// A kept mode below TWO_PASS_RATIO of the largest: deflated levels instead of one Gram pass.
bool rt_deep(const std::vector<double>& s, int r);

// Modes a deflated level accepts from its singular values `sig`: those within LEVEL_RATIO of the largest, at least one,
// at most `room`; none below the floor n eps first_sigma (`have` modes accepted so far, the first of them first_sigma).
int rt_level_size(const std::vector<double>& sig, int have, double first_sigma, int room);

// The spectrum after a level that accepted k modes: s_acc (this level's included), then the level's tail sig[k:] as far as
// n entries go, zeros beyond; energy over `total`.  Returns the length of the tail.
int rt_merged_spectrum(const std::vector<double>& s_acc, const std::vector<double>& sig, int k, double total,
                       std::vector<double>& s_full, std::vector<double>& e_full);

// The levels stop: the kept modes are covered, the level accepted nothing, the spectrum or the level budget is used up,
// or nothing but zeros is left (tail0: the first of the tail, 0 when it is empty).
bool rt_levels_done(int r, int got, int k, int n, int levels, int tail_n, double tail0);

// H c = theta S c for symmetric H and positive definite S (k x k row-major): C = eigenvectors as columns, theta descending.
// False if S is not positive definite.  H and S are not modified.
bool rt_small_generalised_eigh(std::vector<double>& H, std::vector<double>& S, int k, std::vector<double>& C,
                               std::vector<double>& theta);
