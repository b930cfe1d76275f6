"""The POD's decisions from a spectrum are stated once per language - romtime_amd/pod_rules.py and csrc/host_dense.{h,cpp} -
and have to agree.  About 300 seeded cases (n = 3 .. 16) go through both: the C++ side as tests/host/host_dense_check.cpp
with a case file, built stand-alone with g++ and the address and undefined-behaviour sanitizers as
tests/test_host_sanitizers.py builds it.  Integers and booleans must be equal; the merged spectrum and its energy agree to
4 ulp (C sums the trace one term after the other, NumPy may sum pairwise).

The same cases hold ``pod_rules.single_pass_rank`` against the acceptance tests PodPipeline._finish and PodLanes._finish
spelt out before they shared it (copied below as the oracle); on a NaN among the eigenvalues it decides, it rejects."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)
TWO_PASS_RATIO, RR_GAP, LEVEL_RATIO, DROP_TOLERANCE = 1e-2, 1e-4, 0.08, 1e-7   # restated, as tests/svd_cases.py does


def _rules():
    """pod_rules on its own: it needs neither torch nor the built library (the package's __init__ wants torch)."""
    import importlib.util

    name = "_pod_rules_under_test"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "romtime_amd", "pod_rules.py"))
        sys.modules[name] = mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert "torch" not in mod.__dict__
    return sys.modules[name]


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _spectrum(rng, kind, n):
    """Eigenvalues of a Gram matrix (descending), by family."""
    if kind == "shallow":
        s = rng.uniform(0.5, 2.0) * np.cumprod(np.r_[1.0, rng.uniform(0.55, 0.95, n - 1)])
    elif kind == "deep":
        s = rng.uniform(0.5, 2.0) * np.cumprod(np.r_[1.0, 10.0 ** -rng.uniform(0.3, 3.0, n - 1)])
    elif kind == "repeated":      # a repeated eigenvalue among the leading ones
        s = rng.uniform(0.5, 2.0) * np.cumprod(np.r_[1.0, rng.uniform(0.55, 0.95, n - 1)])
        j = rng.randint(0, 2)
        s[j + 1] = s[j]
    elif kind == "zero_tail":     # numerical rank q, an exactly zero tail
        q = rng.randint(1, n)
        s = np.r_[rng.uniform(0.5, 2.0) * np.cumprod(np.r_[1.0, rng.uniform(0.3, 0.9, q - 1)]), np.zeros(n - q)]
    elif kind == "zero":
        s = np.zeros(n)
    else:
        raise ValueError(kind)
    return s * s


def _on_an_edge(c):
    """Why this case is within a relative 1e-6 of a rule's edge (or an energy within 10 % of 1 - tol of tol); '' if not."""
    lam, n, num, tol = c["lam"], c["n"], c["num"], c["tol"]
    if not np.all(np.isfinite(lam)):
        return ""       # a NaN decides by being one, not by a rounding
    s = np.sqrt(np.clip(lam, 0.0, None))

    def near(a, b):
        a = np.asarray(a, dtype=float)
        return bool(np.any(np.abs(a - b) <= 1e-6 * np.maximum(np.abs(a), abs(b)))) if b != 0 else False

    first = c["first"]
    total0 = np.sum(s * s)
    spectra = [(s, total0)]
    if near(s, TWO_PASS_RATIO * s[0]) or near(s, LEVEL_RATIO * s[0]):
        return "a singular value on the shallow/deep or the level edge"
    gaps = np.r_[lam[:-1] - lam[1:], lam[-1]]
    if near(gaps, RR_GAP * max(lam[0], 1e-300)):
        return "a gap on the Rayleigh-Ritz edge"
    if not num and not tol and near(s, DROP_TOLERANCE):
        return "a singular value on the drop rule"
    if first is not None and near([s[0]], n * EPS * first):
        return "the level's largest on the floor"
    if tol and total0 > 0:
        if first is not None:
            spectra = [(s, total0), (np.r_[first, s][:n], first * first + total0)]
        for sp, tot in spectra:
            if np.any(np.abs(np.cumsum(sp * sp) / tot - tol) <= 0.1 * (1.0 - tol)):
                return "an energy within 10 % of 1 - tol of tol"
    return ""


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(20261)
    kinds = ["shallow"] * 4 + ["deep"] * 3 + ["repeated"] * 2 + ["zero_tail"] * 2 + ["zero"]
    out, tags = [], set()
    while len(out) < 300:
        n = int(rng.randint(3, 17))
        kind = kinds[len(out) % len(kinds)] if len(out) % 25 else "zero"
        lam = _spectrum(rng, kind, n)
        cut = rng.randint(3)
        num = int(rng.randint(1, n + 3)) if cut == 0 else 0
        tol = float(1.0 - 10.0 ** -rng.uniform(1.0, 12.0)) if cut == 1 else 0.0
        k = min(num, n) if num else int(rng.randint(1, n + 1))       # what the runners enqueue ahead
        if rng.rand() < 0.15:
            k, num = n, (n if num else 0)
        status = int(rng.rand() < 0.1) * int(rng.randint(1, 4))
        n_rows = int(rng.randint(1, n)) if rng.rand() < 0.1 else int(n + rng.randint(0, 50))
        # a level: nothing accepted yet, or one mode 10^u above this level's largest (u up to 17: over the n eps floor)
        first = None if rng.rand() < 0.4 else float(np.sqrt(max(lam[0], 1e-40)) * 10.0 ** rng.uniform(0.2, 17.0))
        have = 0 if first is None else 1
        room = 0 if rng.rand() < 0.1 else int(rng.randint(0, n - have + 1))
        if kind in ("shallow", "deep") and rng.rand() < 0.12:
            # among the eigenvalues the verdict looks at: lam[1 .. r], r >= 1 whatever the truncation rule
            lam = lam.copy()
            lam[1] = np.nan
        c = dict(n=n, lam=lam, num=num, tol=tol, k=k, status=status, n_rows=n_rows, room=room, first=first, kind=kind)
        if _on_an_edge(c):
            continue        # drawn again; the assertion below is what the comparison rests on
        out.append(c)
    for c in out:
        assert not _on_an_edge(c), (_on_an_edge(c), c)
        lam, n = c["lam"], c["n"]
        fin = bool(np.all(np.isfinite(lam)))
        s = np.sqrt(np.clip(lam, 0.0, None))
        tags.update(t for t, hit in {
            "k == n": c["k"] == n, "all-zero": not lam.any(), "repeated": c["kind"] == "repeated",
            "deep": fin and s[0] > 0 and s[min(c["k"], n) - 1] < TWO_PASS_RATIO * s[0],
            "num above the rank": c["kind"] == "zero_tail" and c["num"] > np.count_nonzero(lam),
            "room == 0": c["room"] == 0, "status != 0": c["status"] != 0, "n_rows < n": c["n_rows"] < n,
            "NaN": not fin, "num": bool(c["num"]), "tol": bool(c["tol"]), "neither": not c["num"] and not c["tol"],
            "first": c["first"] is not None, "under the floor": c["first"] is not None and s[0] <= n * EPS * c["first"],
        }.items() if hit)
    missing = {"k == n", "all-zero", "repeated", "deep", "num above the rank", "room == 0", "status != 0", "n_rows < n", "NaN",
               "num", "tol", "neither", "first", "under the floor"} - tags
    assert not missing, missing
    return tuple(out)


# ---- the Python side ---------------------------------------------------------------------------------------------------------
def python_decisions(c):
    R = _rules()
    lam, n, num, tol = c["lam"], c["n"], c["num"] or None, c["tol"] or None
    with np.errstate(all="ignore"):
        s = R.sigma(lam)
        r = R.truncation_rank(s, R.energy(s), num=num, tol=tol)
        sep = bool(r > 0 and R.separated(lam, r))
        verdict = R.single_pass_rank(lam, c["status"], c["n_rows"], c["k"], num=num, tol=tol)
        first = c["first"]
        accepted = [] if first is None else [np.array([first])]
        total = float(np.sum(np.clip(lam, 0.0, None))) + (0.0 if first is None else first * first)   # as _pod_deflated
        kl = R.level_size(s, first, c["room"], n)
        if kl > 0:
            accepted.append(s[:kl])
        s_full, e_full, tail = R.merged_spectrum(accepted, s, kl, total)
        r_after = R.truncation_rank(s_full, e_full, num=num, tol=tol)
        stop = R.levels_done(r_after, sum(len(x) for x in accepted), kl, n, 1, tail)
    return dict(ints=[r, int(R.deep(s, r)), int(sep), -1 if verdict is None else verdict, kl, r_after, int(stop)],
                s=s_full, energy=e_full)


def _ulps(a, b):
    """Distance in units of the last place; two NaNs (the energy of an all-zero spectrum) are no distance apart."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
    d = np.where(a == b, 0.0, d)
    return np.where(both_nan, 0.0, np.where(np.isnan(d), np.inf, d))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cxx_and_python_rules_decide_alike(tmp_path):
    exe, path = str(tmp_path / "host_dense_check"), str(tmp_path / "cases.txt")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(REPO, "tests", "host", "host_dense_check.cpp"), os.path.join(REPO, "romtime_amd", "csrc", "host_dense.cpp"),
           "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    with open(path, "w") as f:
        for c in cases():
            head = [c["n"], c["num"], float(c["tol"]).hex(), c["k"], c["status"], c["n_rows"], c["room"],
                    float(-1.0 if c["first"] is None else c["first"]).hex()]
            f.write(" ".join(str(v) for v in head + [float(v).hex() for v in c["lam"]]) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(cases())
    worst = 0.0
    for c, line in zip(cases(), lines):
        ints, levels, s_txt, e_txt = (part.split() for part in line.split("|"))
        got = [int(v) for v in ints + levels]
        want = python_decisions(c)
        assert got == want["ints"], (c, got, want["ints"])
        d = max(_ulps([float.fromhex(v) for v in s_txt], want["s"]).max(),
                _ulps([float.fromhex(v) for v in e_txt], want["energy"]).max())
        worst = max(worst, d)
        assert d <= 4.0, (c, d, line, want)
    print(f"POD-RULES {len(lines)} cases, C++ against Python: integers equal, s and energy within {worst:.2f} ulp")


# ---- the acceptance tests of the two runners as they stood, each in its own words -----------------------------------------------
def _pipeline_finish_before(lam, status, n_rows, k):
    n = len(lam)
    s = np.sqrt(np.clip(lam, 0.0, None))
    gaps = lam[:k] - lam[1:k + 1] if k < n else np.r_[lam[:k - 1] - lam[1:k], lam[k - 1]]
    ok = (status == 0 and s[0] > 0 and s[k - 1] >= TWO_PASS_RATIO * s[0]
          and gaps.min() >= RR_GAP * max(lam[0], 1e-300) and n_rows >= n)
    return k if ok else None


def _lanes_finish_before(lam, status, n_rows, k, num, tol):
    n = len(lam)
    s = np.sqrt(np.clip(lam, 0.0, None))
    ev = np.power(s, 2)
    energy = np.cumsum(ev) / np.sum(ev)
    r = int(np.count_nonzero(energy < tol)) if tol else (int(min(num, n)) if num else int(np.count_nonzero(s > DROP_TOLERANCE)))
    if status != 0 or not (1 <= r <= k) or not s[0] > 0 or n_rows < n:
        return None
    gaps = lam[:r] - lam[1:r + 1] if r < n else np.r_[lam[:r - 1] - lam[1:r], lam[r - 1]]
    if s[r - 1] < TWO_PASS_RATIO * s[0] or gaps.min() < RR_GAP * max(lam[0], 1e-300):
        return None
    return r


def test_single_pass_rank_is_what_the_runners_decided():
    R = _rules()
    seen = {"pipeline": 0, "lanes": 0, "accepted": 0, "nan": 0}
    with np.errstate(all="ignore"):
        for c in cases():
            lam, n, num, tol = c["lam"], c["n"], c["num"] or None, c["tol"] or None
            # PodLanes: with `num` alone it enqueues min(num, n) vectors, else `cap` of them (the case's k)
            new = R.single_pass_rank(lam, c["status"], c["n_rows"], c["k"], num=num, tol=tol)
            if not np.all(np.isfinite(lam)):
                assert new is None, c
                seen["nan"] += 1
                continue
            assert new == _lanes_finish_before(lam, c["status"], c["n_rows"], c["k"], num, tol), c
            seen["lanes"] += 1
            seen["accepted"] += new is not None
            if num and not tol:      # PodPipeline takes `num` alone, and k = min(num, n)
                assert c["k"] == min(num, n)
                assert new == _pipeline_finish_before(lam, c["status"], c["n_rows"], c["k"]), c
                seen["pipeline"] += 1
    assert seen["pipeline"] >= 50 and seen["lanes"] >= 200 and seen["accepted"] >= 30 and seen["nan"] >= 5, seen
