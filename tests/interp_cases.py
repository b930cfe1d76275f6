"""Shared pieces of the interpolation-certification tests (tests/test_interpolation_cpu.py, tests/test_interpolation_gpu.py):
a NumPy restatement of ``ops.interpolation_errors``, the launch plan of rt_interpolation_errors restated, the truth in
np.longdouble, the error bar, and the case builders - exact integer data, random graded bases with snapshots that leave the
span by 1e-3, and three mock reductors.  Plain module, not a conftest.

The bar, per snapshot:   bar_s = 16 m^(3/2) eps cond_2(PT_U) ||PT_U^-1||_2 ||f_s||_2 / sqrt(N)
the forward error of an LU solve for Psi = basis_fom PT_U^-1 (m eps cond_2 per entry, relative to the basis) followed by
a length-m dot product per entry of the interpolant (sqrt(m) ||f[idx]||_2 <= sqrt(m) ||f||_2, the solved rows at most
||PT_U^-1||_2 for a basis with rows of at most unit norm), with slack 16.  A group's bar is the mean of its snapshots'."""
import numpy as np
import torch

EPS = float(np.finfo(np.float64).eps)
SLACK = 16.0


def _cdiv(a, b):
    return -(-a // b)


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def group_mean(e, group):
    """The reference's mean over the states (nonlinear.py:518-535): a running float64 sum in index order, one division."""
    e = np.asarray(e, dtype=np.float64)
    out = np.empty(e.size // group)
    for q in range(out.size):
        acc = 0.0
        for i in range(group):
            acc = acc + e[q * group + i]
        out[q] = acc / float(group)
    return out


def numpy_interpolation_errors(Psi, idx, F, group=1, pin=None, want_ref=False):
    """What ops.interpolation_errors computes, in NumPy float64 (monkeypatched over it in the host-logic tests): the
    product, (f - l), the square, the column sums, sqrt, the division and the running group mean as separate operations."""
    Pn, Fn = _np(Psi), _np(F)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    N = Pn.shape[0]
    assert idx.size == Pn.shape[1] and Fn.shape[0] == N and Fn.shape[1] % group == 0
    assert idx.min() >= 0 and idx.max() < N
    C = Fn[idx, :]
    L = np.stack([Pn @ C[:, s] for s in range(Fn.shape[1])], axis=1)      # column by column: a snapshot's value does
    if pin is not None:                                                     # not depend on the block it arrives in
        L[int(pin[0]), :] = float(pin[1])
    d = Fn - L
    colsum = lambda a: np.array([np.sum(np.ascontiguousarray(a[:, s])) for s in range(a.shape[1])])
    err = group_mean(np.sqrt(colsum(d * d)) / np.sqrt(float(N)), group)
    if not want_ref:
        return torch.from_numpy(err)
    ref = group_mean(np.sqrt(colsum(Fn * Fn)) / np.sqrt(float(N)), group)
    return torch.from_numpy(err), torch.from_numpy(ref)


def numpy_dense_solve_multi(K, B):
    """ops.dense_solve_multi on CPU tensors: (X, info) with info != 0 for a zero pivot of the partial-pivoting LU."""
    from scipy.linalg import lu_factor, lu_solve

    Kn, Bn = _np(K), _np(B)
    with np.errstate(all="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lu = lu_factor(Kn, check_finite=False)
    if np.any(np.diag(lu[0]) == 0.0):
        return torch.zeros(Bn.shape, dtype=torch.float64), torch.ones(1, dtype=torch.int32)
    return torch.from_numpy(lu_solve(lu, Bn)), torch.zeros(1, dtype=torch.int32)


def numpy_p1_local_assembly(kind, nx, rows, cols, h, coef=None, state=None, ramp=None, poly=None):
    """ops.p1_local_assembly for the mass and the stiffness, through the mock FOM's own entry-wise assembly."""
    from romtime_amd.testing.mock import MockSolver

    assert kind in ("mass", "stiffness") and state is None and ramp is None and poly is None
    solver = MockSolver(domain={"L0": 1.0, "nx": int(nx), "T": 1.0, "nt": 1})
    solver.setup()
    entries = list(zip(_np(rows).tolist(), _np(cols).tolist()))
    hn = np.atleast_1d(_np(h))
    cn = np.ones(hn.size) if coef is None else np.atleast_1d(_np(coef))
    ref = np.array([[2.0, 1.0], [1.0, 2.0]]) if kind == "mass" else np.array([[1.0, -1.0], [-1.0, 1.0]])
    out = np.empty((hn.size, len(entries)))
    for s in range(hn.size):
        scale = hn[s] / 6.0 if kind == "mass" else cn[s] / hn[s]
        out[s] = solver._assemble_matrix(np.tile(scale * ref, (int(nx), 1, 1)), entries)
    return torch.from_numpy(out)


def interpolation_errors_plan(N, S, cus):
    """launch_info of rt_interpolation_errors (interp_error.hip): the row slices depend on N and the CU count only."""
    step_blocks = _cdiv(S, 64)
    slices = min(cus, _cdiv(N, 1024))
    slice_rows = _cdiv(_cdiv(N, slices), 32) * 32
    slices = _cdiv(N, slice_rows)
    return dict(grid=step_blocks * slices, splits=slices, tile=(32, 64))


# ---- truth and bar ---------------------------------------------------------------------------------------------------

def longdouble_thetas(PT_U, rhs):
    """solve(PT_U, rhs) to long-double accuracy: the float64 LU refined against residuals formed in np.longdouble."""
    from scipy.linalg import lu_factor, lu_solve

    ld = np.longdouble
    A = np.asarray(PT_U, dtype=np.float64)
    lu = lu_factor(A)
    Al, bl = A.astype(ld), np.asarray(rhs, dtype=np.float64).astype(ld)
    x = lu_solve(lu, np.asarray(rhs, dtype=np.float64)).astype(ld)
    for _ in range(6):
        r = bl - Al @ x
        x = x + lu_solve(lu, r.astype(np.float64)).astype(ld)
    assert np.abs(bl - Al @ x).max() <= 64 * float(np.finfo(ld).eps) * (np.abs(Al) @ np.abs(x)).max() + 1e-300
    return x


def longdouble_errors(basis, PT_U, idx, F, pin=None, group=1):
    """err of rt_interpolation_errors' definition with I(f) = basis solve(PT_U, f[idx]), everything in np.longdouble on
    the float64 inputs: thetas, product, pin, norm and group mean."""
    ld = np.longdouble
    Fn = np.asarray(F, dtype=np.float64)
    theta = longdouble_thetas(PT_U, Fn[np.asarray(idx), :])
    L = np.asarray(basis, dtype=np.float64).astype(ld) @ theta
    if pin is not None:
        L[int(pin[0]), :] = ld(pin[1])
    d = Fn.astype(ld) - L
    e = np.sqrt(np.sum(d * d, axis=0)) / np.sqrt(ld(Fn.shape[0]))
    return e.reshape(-1, group).sum(axis=1) / ld(group) if group > 1 else e


def error_bar(PT_U, F, group=1):
    """bar_s of the module docstring for every snapshot (column) of F; with ``group`` the mean over each group."""
    Fn = np.asarray(F, dtype=np.float64)
    N, m = Fn.shape[0], np.shape(PT_U)[0]
    s = np.linalg.svd(np.asarray(PT_U, dtype=np.float64), compute_uv=False)
    bar = SLACK * m ** 1.5 * EPS * (s[0] / s[-1]) * (1.0 / s[-1]) * np.linalg.norm(Fn, axis=0) / np.sqrt(float(N))
    return bar.reshape(-1, group).mean(axis=1) if group > 1 else bar


def oracle_errors(basis, PT_U, idx, F, pin=None, group=1):
    """The reference's arithmetic in float64: oracle.interpolate + oracle.compute_error per snapshot, the running mean."""
    from oracle import romtime_oracle as oracle

    Fn = np.asarray(F, dtype=np.float64)
    e = []
    for s in range(Fn.shape[1]):
        approx = oracle.interpolate(basis, PT_U, Fn[np.asarray(idx), s])
        if pin is not None:
            approx[int(pin[0])] = float(pin[1])
        e.append(oracle.compute_error(approx, Fn[:, s]))
    return group_mean(e, group)


# ---- exact data ------------------------------------------------------------------------------------------------------

PSI_BITS, F_BITS = 3, 6          # |Psi| <= 8, |F| <= 64: |l| <= 128 * 2^9, (f - l)^2 < 2^35, a column sum of 2081 < 2^47

EXACT_CASES = [
    # id, N, S, m, layout of F, (ldpsi, ldf) padding, misaligned, pin_row, pin_value, group, want_ref
    ("one_word", 1, 1, 1, "F", (0, 0), False, -1, 0.0, 1, True),
    ("one_row_pinned_group_all", 1, 63, 1, "C", (1, 1), True, 0, 1.0, 63, False),
    ("one_row_m3", 1, 130, 3, "F", (2, 0), False, 0, 3.0, 5, True),
    ("n31_m3_group5", 31, 65, 3, "F", (2, 1), True, 0, 1.0, 5, True),
    ("n31_m81_single", 31, 1, 81, "C", (0, 2), False, 30, -2.0, 1, False),
    ("n33_m4_rowmajor_pin32", 33, 130, 4, "C", (0, 3), False, 32, 1.0, 1, False),
    ("n33_m5_pin31", 33, 63, 5, "F", (1, 0), False, 31, 1.0, 1, True),
    ("n1023_m1_rowmajor_pin31", 1023, 63, 1, "C", (1, 0), True, 31, 1.0, 63, True),
    ("n1023_m81_pin_last", 1023, 130, 81, "F", (0, 1), True, 1022, 1.0, 5, True),
    ("n1025_m127_rowmajor_pin1023", 1025, 65, 127, "C", (1, 1), True, 1023, 5.0, 65, False),
    ("n1025_m128_single_pin1024", 1025, 1, 128, "F", (0, 0), False, 1024, 1.0, 1, True),
    ("n2081_m128_rowmajor_slices", 2081, 63, 128, "C", (3, 2), False, -1, 0.0, 1, True),
    ("n2081_m5_pin1024_group_all", 2081, 130, 5, "F", (0, 0), False, 1024, 1.0, 130, True),
    ("n2081_m4_misaligned_pin32", 2081, 65, 4, "F", (1, 3), True, 32, 1.0, 5, False),
    ("n2081_m127_rowmajor_pin_last", 2081, 130, 127, "C", (0, 1), True, 2080, 1.0, 1, False),
]


def exact_case(case):
    """Integer Psi (N x m), F (N x S) and indices that hold 0, N - 1 and the pinned row."""
    from tests.guarded import exact_operands

    _, N, S, m, _, _, _, pin_row, _, _, _ = case
    rng = np.random.default_rng(N * 1_000_003 + S * 1009 + m * 31 + pin_row + 7)
    Psi = exact_operands(rng, (N, m), PSI_BITS)
    F = exact_operands(rng, (N, S), F_BITS)
    idx = rng.integers(0, N, size=m).astype(np.int64)
    special = [0, N - 1] + ([pin_row] if pin_row >= 0 else [])
    for slot, value in zip(rng.permutation(m)[:len(special)], special):
        idx[slot] = value
    return Psi, idx, F


def exact_sums(Psi, idx, F, pin):
    """(sum (f - l)^2, sum f^2) per snapshot in integer arithmetic (int64, no rounding; every value checked below 2^53)."""
    Pi, Fi = Psi.astype(np.int64), F.astype(np.int64)
    assert np.array_equal(Pi, Psi) and np.array_equal(Fi, F)
    L = Pi @ Fi[idx, :]
    if pin is not None:
        assert float(pin[1]) == int(pin[1])
        L[int(pin[0]), :] = int(pin[1])
    d = Fi - L
    assert np.abs(L).max() < 2 ** 26 and np.abs(d).max() < 2 ** 26
    se, sr = np.sum(d * d, axis=0), np.sum(Fi * Fi, axis=0)
    assert int(se.max()) < 2 ** 53 and int(sr.max()) < 2 ** 53
    return se, sr


def exact_expected(case, Psi, idx, F):
    """(err, ref) of an exact case: correctly rounded sqrt and division of exact integers, then the running mean."""
    _, N, S, m, _, _, _, pin_row, pin_value, group, _ = case
    se, sr = exact_sums(Psi, idx, F, None if pin_row < 0 else (pin_row, pin_value))
    err = group_mean(np.sqrt(se.astype(np.float64)) / np.sqrt(float(N)), group)
    ref = group_mean(np.sqrt(sr.astype(np.float64)) / np.sqrt(float(N)), group)
    return err, ref


# ---- random data -----------------------------------------------------------------------------------------------------

RANDOM_CASES = [
    # id, N, m, S, pin, group
    ("n2081_m24", 2081, 24, 130, None, 1),
    ("n4099_m81_pinned", 4099, 81, 70, (0, 1.0), 1),
    ("n1040_m128_grouped", 1040, 128, 65, (0, 1.0), 5),
]
SMALL_RANDOM = ("n97_m5", 97, 5, 20, None, 1)     # CPU only: the fourth shape the bar was checked on

_random_cache = {}


def random_case(case):
    """A graded basis (orthonormal columns scaled by sqrt(N) 2^(-3 j / m): rows of PT_U are O(1)), ``oracle.deim_greedy``
    points, and snapshots basis c + 1e-3 ||basis c|| (unit noise): they leave the span by 1e-3.  Cached: built once."""
    if case[0] in _random_cache:
        return _random_cache[case[0]]
    from oracle import romtime_oracle as oracle

    _, N, m, S, pin, group = case
    rng = np.random.default_rng(N * 7919 + m)
    Q, _ = np.linalg.qr(rng.standard_normal((N, m)))
    basis = np.ascontiguousarray(Q * (np.sqrt(float(N)) * 2.0 ** (-3.0 * np.arange(m) / m))[None, :])
    dofs, PT_U, _ = oracle.deim_greedy(basis)
    inside = basis @ rng.standard_normal((m, S))
    noise = rng.standard_normal((N, S))
    noise /= np.linalg.norm(noise, axis=0)[None, :]
    F = inside + 1e-3 * np.linalg.norm(inside, axis=0)[None, :] * noise
    resid = F - basis @ np.linalg.lstsq(basis, F, rcond=None)[0]
    off_span = np.linalg.norm(resid, axis=0) / np.linalg.norm(F, axis=0)
    if pin is not None:
        F[int(pin[0]), :] = pin[1] + 1e-3 * rng.standard_normal(S)      # a Dirichlet entry: near its pinned value
    out = dict(off_span=off_span,basis=basis, PT_U=np.ascontiguousarray(PT_U), idx=np.asarray(dofs, dtype=np.int64), F=np.ascontiguousarray(F),
               pin=pin, group=group)
    out["truth"] = longdouble_errors(basis, out["PT_U"], out["idx"], F, pin, group)
    out["bar"] = error_bar(out["PT_U"], F, group)
    out["Psi"] = np.ascontiguousarray(np.linalg.solve(out["PT_U"].T, basis.T).T)
    _random_cache[case[0]] = out
    return out


# ---- mock reductors --------------------------------------------------------------------------------------------------

MOCK_CASES = ("mass", "stiffness_ale", "trilinear")
MOCK_TS = [0.3, 1.1, 2.4, 3.7]
MOCK_MUS = [dict(alpha_0=1.3, delta=0.35, omega=9.0), dict(alpha_0=0.8, delta=0.8, omega=10.5)]
_TRAIN_MUS = [dict(alpha_0=a, delta=d, omega=9.5) for a, d in ((0.6, 0.2), (1.0, 0.5), (1.5, 0.9))]
_TRAIN_TS = [0.5, 1.5, 2.5, 3.5, 4.5]


def mock_solver(nx=60):
    from romtime_amd.testing.mock import MockBurgers

    solver = MockBurgers(domain={"L0": 1.0, "nx": nx, "T": 5.0, "nt": 100}, Lt=lambda t, **mu: 1.0 + 0.1 * mu["delta"] * t)
    solver.setup()
    return solver


def mock_states(nx=60):
    """Three strictly increasing nodal states: every entry of the trilinear operator's topology stays nonzero."""
    x = np.linspace(0.0, 1.0, nx + 1)
    return np.stack([(1.0 + x) ** (k + 1) for k in range(3)], axis=1)


def mock_reductor(which, nx=60):
    """A reductor of the mock FOM with a truncated collateral basis (``load_fom_basis(keep=...)``), built from a host SVD of
    a few training snapshots; the caller's ``ops`` (device, or the CPU stand-ins) run the greedy.  Returns
    (reductor, solver)."""
    from romtime_amd import MatrixDiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolationNonlinear

    solver = mock_solver(nx)
    rnd = np.random.RandomState(0)
    from scipy.stats.distributions import uniform

    grid = dict(alpha_0=uniform(0.5, 1.0), delta=uniform(0.1, 0.8), omega=uniform(8.5, 3.0))
    if which == "trilinear":
        red = MatrixDiscreteEmpiricalInterpolationNonlinear(name="trilinear", assemble=solver.assemble_trilinear, grid=grid)
        red.setup(rnd=rnd, u_n=np.linspace(0.0, 1.0, solver.Nh))
        red.u_n = mock_states(nx)
        train = mock_states(nx) @ np.array([[1.0, 0.2, 0.5, 0.1], [0.3, 1.0, 0.2, 0.7], [0.1, 0.4, 1.0, 0.9]])
        snaps = [red.assemble_snapshot(mu=_TRAIN_MUS[0], t=1.0, u_n=train[:, i]) for i in range(train.shape[1])]
        keep = 2
    else:
        assemble = solver.assemble_mass if which == "mass" else solver.assemble_stiffness
        red = MatrixDiscreteEmpiricalInterpolation(name=which, assemble=assemble, grid=grid)
        red.setup(rnd=rnd)
        snaps = [red.assemble_snapshot(mu, t) for mu in _TRAIN_MUS for t in _TRAIN_TS]
        keep = 1
    X = np.array(snaps).T
    X[0, :] = 0.0                                                     # the MDEIM convention of the tree walk (deim.py:388-389)
    U, s, _ = np.linalg.svd(X, full_matrices=False)
    assert s[keep] > 1e-8 * s[0], s                                   # the truncation drops something: errors are not rounding
    red.load_fom_basis(keep=keep, basis=np.ascontiguousarray(U[:, :keep + 1]))
    return red, solver


def mock_samples(red, mu, ts):
    """The exact snapshots ``evaluate`` certifies for one parameter point, as columns, and the group size."""
    if red.TYPE == "N-MDEIM":
        cols = [red.assemble_snapshot(mu=mu, t=t, u_n=red.u_n[:, i]) for t in ts for i in range(red.u_n.shape[1])]
        return np.array(cols).T, red.u_n.shape[1]
    return np.array([red.assemble_snapshot(mu, t) for t in ts]).T, 1
