// CPU-side sanitizer run of the library's host code (romtime_amd/csrc/host_dense.cpp): built by
// tests/test_host_sanitizers.py with  g++ -fsanitize=address,undefined -fno-sanitize-recover=all  and executed; any heap /
// stack overrun, use of uninitialised-by-construction memory the sanitizers see, signed overflow or misaligned access
// aborts the run.  The numerical checks double as known-answer tests of the three helpers.
//
// With a file name as argument it prints instead what the POD rules of host_dense.h decide on the cases of that file, one
// line per case, for tests/test_pod_rules_cpu.py to hold against romtime_amd/pod_rules.py (formats: `decide` below).
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../romtime_amd/csrc/host_dense.h"

static int fail(const char* what, double v) {
  std::printf("FAIL %s (%g)\n", what, v);
  return 1;
}

// A case is one line "n num tol k status n_rows room first lam[0] .. lam[n-1]" (doubles as hex floats; first < 0: no mode
// accepted yet, else one mode with that singular value was).  Its answer is one line
//   r deep separated(r) verdict | level_size r_after stop | s[0..n) | energy[0..n)
// r .. verdict: `lam` as the spectrum of a whole set - truncation rank, rt_deep, rt_separated (0 when r == 0) and whether
// k single-pass vectors enqueued ahead may be handed out (r, or -1); level_size .. energy: `lam` as the spectrum of a
// deflated level with `room` columns left - what it accepts, the merged spectrum after it, the rank on that, the stop flag.
// The verdict is composed HERE from the library's pieces (rank, sigma, rt_separated) and the shallow bound written out: the
// library has no such function (what rt_pod_enqueue put ahead is judged in Python), so that column holds
// pod_rules.single_pass_rank against this restatement and says nothing about shipped C code; the other columns do.
static int decide(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return fail("cannot open the case file", 0);
  int n, k, status, room;
  long num, n_rows;
  double tol, first;
  while (std::fscanf(f, "%d %ld %la %d %d %ld %d %la", &n, &num, &tol, &k, &status, &n_rows, &room, &first) == 8) {
    std::vector<double> lam(n), energy, s_full, e_full;
    for (double& v : lam)
      if (std::fscanf(f, "%la", &v) != 1) return fail("short case", n);
    const std::vector<double> s = rt_sigma(lam);
    double total = 0.0;
    for (double v : s) total += v * v;
    rt_energy(s, total, energy);
    const int r = rt_truncation_rank(s, energy, num, tol);
    const bool sep = r > 0 && rt_separated(lam, r);
    const bool ok = status == 0 && n_rows >= n && 1 <= r && r <= k && s[0] > 0.0 && s[r - 1] >= RT_TWO_PASS_RATIO * s[0] && sep;
    std::vector<double> s_acc;
    if (first >= 0.0) { s_acc.push_back(first); total = first * first + total; }
    const int have = (int)s_acc.size();
    const int kl = rt_level_size(s, have, have ? s_acc[0] : 0.0, room);
    s_acc.insert(s_acc.end(), s.begin(), s.begin() + kl);
    const int tail_n = rt_merged_spectrum(s_acc, s, kl, total, s_full, e_full);
    const int r_after = rt_truncation_rank(s_full, e_full, num, tol);
    const bool stop = rt_levels_done(r_after, have + kl, kl, n, 1, tail_n, tail_n > 0 ? s[kl] : 0.0);
    std::printf("%d %d %d %d | %d %d %d |", r, (int)rt_deep(s, r), (int)sep, ok ? r : -1, kl, r_after, (int)stop);
    for (double v : s_full) std::printf(" %a", v);
    std::printf(" |");
    for (double v : e_full) std::printf(" %a", v);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return decide(argv[1]);
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd(0.0, 1.0);
  for (int n : {1, 2, 3, 7, 32, 65}) {
    // graded PSD matrix A = B diag(10^-i) B^T
    std::vector<double> B((size_t)n * n), A((size_t)n * n, 0.0), A0;
    for (auto& x : B) x = nd(rng);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += B[(size_t)i * n + k] * std::pow(10.0, -0.5 * k) * B[(size_t)j * n + k];
        A[(size_t)i * n + j] = s;
      }
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) A[(size_t)j * n + i] = A[(size_t)i * n + j];
    A0 = A;
    std::vector<double> W((size_t)n * n), lam(n);
    int sweeps = -1;
    if (rt_host_jacobi_eigh(A.data(), n, W.data(), lam.data(), 60, &sweeps) != RT_OK) return fail("jacobi rc", n);
    double res = 0.0, orth = 0.0, scale = std::fabs(lam[0]) + 1e-300;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double av = 0.0, ww = 0.0;
        for (int k = 0; k < n; ++k) { av += A0[(size_t)i * n + k] * W[(size_t)k * n + j]; ww += W[(size_t)k * n + i] * W[(size_t)k * n + j]; }
        res = std::fmax(res, std::fabs(av - lam[j] * W[(size_t)i * n + j]));
        orth = std::fmax(orth, std::fabs(ww - (i == j ? 1.0 : 0.0)));
      }
    if (res > 1e-12 * scale) return fail("jacobi residual", res);
    if (orth > 1e-12) return fail("jacobi orthogonality", orth);
    for (int i = 0; i + 1 < n; ++i)
      if (lam[i] < lam[i + 1]) return fail("jacobi order", i);
    // generalised problem with S = I + small SPD perturbation
    std::vector<double> H(A0), S((size_t)n * n, 0.0), C, theta;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) S[(size_t)i * n + j] = (i == j ? 1.0 : 0.0) + 1e-3 * A0[(size_t)i * n + j] / scale;
    if (!rt_small_generalised_eigh(H, S, n, C, theta)) return fail("generalised eigh rc", n);
    double gres = 0.0;
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        double hc = 0.0, sc = 0.0;
        for (int k = 0; k < n; ++k) { hc += H[(size_t)i * n + k] * C[(size_t)k * n + j]; sc += S[(size_t)i * n + k] * C[(size_t)k * n + j]; }
        gres = std::fmax(gres, std::fabs(hc - theta[j] * sc));
      }
    if (gres > 1e-11 * scale) return fail("generalised residual", gres);
    std::vector<double> bad(S);
    bad[0] = -1.0;
    if (rt_small_generalised_eigh(H, bad, n, C, theta)) return fail("indefinite S accepted", n);
  }
  if (rt_host_jacobi_eigh(nullptr, 3, nullptr, nullptr, 1, nullptr) != RT_ERR_ARG) return fail("null arguments", 0);
  // truncation rule (pod.py:46-57): tol (strict) > num > drop tolerance
  std::vector<double> s{3.0, 1.0, 1e-3, 5e-8, 0.0}, e(5);
  double tot = 0.0, run = 0.0;
  for (double v : s) tot += v * v;
  for (int i = 0; i < 5; ++i) { run += s[i] * s[i]; e[i] = run / tot; }
  if (rt_truncation_rank(s, e, 0, 0.0) != 3) return fail("drop rule", rt_truncation_rank(s, e, 0, 0.0));
  if (rt_truncation_rank(s, e, 2, 0.0) != 2 || rt_truncation_rank(s, e, 9, 0.0) != 5) return fail("num rule", 0);
  if (rt_truncation_rank(s, e, 2, 0.95) != 1) return fail("tol precedence / strictness", rt_truncation_rank(s, e, 2, 0.95));
  std::printf("host_dense_check ok\n");
  return 0;
}
