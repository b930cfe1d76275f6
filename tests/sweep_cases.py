"""Shared pieces of the sweep truth tests (tests/test_sweep_truth_cpu.py, tests/test_sweep_truth_gpu.py) and the CSR
pattern builders of tests/test_kernels_gpu.py.  Plain host module, not a conftest; nothing here needs a GPU.

The measure is the ONE-STEP DEFECT of a trajectory against its own states.  For every parameter point b and step s take
u^n = uN[b, s-1], u^{n-1} = uN[b, s-2] (zeros before the start), form K_N and b_N in np.longdouble exactly as
include/romtime_hip.h states them above rt_rom_bdf_sweep / rt_hrom_bdf_sweep, and look at d = K_N uN[b, s] - b_N.
Nothing accumulates over the horizon: a fault in a single step, point or table row shows at that step.

    ratio = |d|_inf / floor,   floor = EPS max_i( depth (K_abs |x|)_i + r (|K_N| |x|)_i + (b_abs)_i )

K_abs and b_abs are the same assemblies carried out on the absolute values of every operand (cancellation inside an
assembly is thereby paid for), depth is the longest summation chain of the assembly: M = m_mass + m_lin + m_nl for the
hyper-reduced sweep, the longest row of the pattern + N for the direct one.  The bar is the project's ratio bar
(tests/solve_cases.py): ratio_device <= F max(ratio_numpy, 1), where ratio_numpy is the same measure for a plain float64
NumPy restatement of that one step from the same two states, solved with np.linalg.solve.

``hrom_case`` / ``direct_case`` build the models, ``assemble`` is the step (long double or float64, optionally with a
planted fault), ``play`` iterates it in float64 (NumPy playing the device), ``play_longdouble`` iterates it in long
double with a Gaussian elimination of its own (the cross-check against the oracle), ``measure`` is the measure."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
from scipy.sparse import csr_matrix

from tests.solve_cases import EPS, synthetic_hrom_terms

LD = np.longdouble

# The ratio bar of the two sweeps: ten times the worst ratio_device / max(ratio_numpy, 1) measured on an MI355X over all
# cases of tests/test_sweep_truth_gpu.py, never more than 100.  NumPy's own ratio stayed below 0.12 on every step of
# every case, so max(ratio_numpy, 1) = 1 and the worst quotient is the worst device ratio:
#   hyper-reduced 0.275 (size_r2, BDF1; then lin_none_r11 0.208, graph rhs_two 0.174, size_r1 0.173, points_32 0.154)
#   direct        0.213 (N_3_r1, BDF2; then square_r16 0.055, N_3_r1 BDF1 0.048, rhs_three 0.041)
F_HSWEEP = 2.75
F_SWEEP = 2.13
GMRES_TOL = 1e-10  # atol and rtol of RomConstructor.GMRES_OPTIONS (the reference's rom.py:36)


# ---- CSR patterns ------------------------------------------------------------------------------------------------------
def penta(N, rng):
    offs = [-2, -1, 0, 1, 2]
    rows, cols = [], []
    for o in offs:
        i = np.arange(max(0, -o), min(N, N - o))
        rows.append(i)
        cols.append(i + o)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = csr_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(N, N))
    A.sort_indices()
    return A


PATTERNS = ("ragged_band", "wide", "mixed", "empty_rows")


def pattern_matrix(pattern, N, rng):
    """The patterns the banded matrices do not reach: rows of unequal length inside a window, a pattern no stage of
    which can be windowed, one where a few stages can not, empty rows."""
    if pattern == "ragged_band":
        A = penta(N, rng).tolil()
        drop = rng.rand(N) < 0.3
        for i in np.nonzero(drop)[0]:
            if 2 <= i < N - 2:
                A[i, i - 2] = 0.0
                A[i, i + 1] = 0.0
        A = csr_matrix(A)
    elif pattern == "wide":
        rows = np.repeat(np.arange(N), 6)
        cols = rng.randint(0, N, size=rows.size)
        A = csr_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(N, N))
    elif pattern == "mixed":
        A = penta(N, rng).tolil()
        for i in rng.choice(N, size=12, replace=False):
            A[i, (i + N // 2) % N] = 1.5
        A = csr_matrix(A)
    elif pattern == "empty_rows":
        A = penta(N, rng).tolil()
        for i in (0, 5, 6, 7, min(500, N - 2), N - 1):
            A[i, :] = 0.0
        A = csr_matrix(A)
    else:
        raise ValueError(pattern)
    A.eliminate_zeros()
    A.sum_duplicates()
    A.sort_indices()
    return A


# ---- hyper-reduced models -----------------------------------------------------------------------------------------------
def identity_terms(mass, lin, nl, rhs):
    """The same operators with PT_U = I: F becomes theta = F PT_U (PT_U is orthogonal), so that the fold of
    ``hrom_bdf_sweep`` solves against the identity and Z = basis_rom^T bit for bit."""
    def one(t):
        m = t["PT_U"].shape[0]
        return dict(t, PT_U=np.eye(m), F=np.ascontiguousarray(t["F"] @ t["PT_U"]))
    nl2 = None if nl is None else dict(nl, PT_U=np.eye(nl["PT_U"].shape[0]))
    return one(mass), [one(t) for t in lin], nl2, [one(t) for t in rhs]


def hrom_case(seed, r, bdf2, nt=4, n_mu=3, m_mass=4, lin=((3, "spd"), (5, "general")), m_nl=6, nl="full", n_rhs=1, m_rhs=4,
              dt=0.05):
    """A hyper-reduced model with PT_U = I on top of ``synthetic_hrom_terms`` (whose draws for a given generator state
    are untouched).  ``nl``: "full", "noC", "noS", "bare" (neither) or None; ``lin``: () for no linear term; ``n_rhs``:
    0 for no source (further source terms are drawn after the generator's own)."""
    rng = np.random.RandomState(seed)
    mass, lin_t, nl_t, rhs_t = identity_terms(*synthetic_hrom_terms(rng, r, nt, n_mu, m_mass, list(lin), max(m_nl, 1), m_rhs))
    for _ in range(1, n_rhs):
        rhs_t.append(dict(PT_U=np.eye(m_rhs), basis_rom=rng.standard_normal((r, m_rhs)), F=rng.standard_normal((nt, n_mu, m_rhs))))
    rhs_t = rhs_t[:n_rhs]
    if nl is None:
        nl_t = None
    else:
        nl_t = dict(nl_t, C=nl_t["C"] if nl in ("full", "noS") else None, S=nl_t["S"] if nl in ("full", "noC") else None)
    blocks = [mass] + lin_t + ([nl_t] if nl_t is not None else [])
    cat = lambda ts: np.ascontiguousarray(np.concatenate([t["F"] for t in ts], axis=2)) if ts else None
    c = SimpleNamespace(kind="hrom", r=r, n_mu=n_mu, nt=nt, dt=dt, bdf2=bool(bdf2), mm=m_mass,
                        ml=sum(t["F"].shape[2] for t in lin_t), mn=0 if nl_t is None else nl_t["W"].shape[0],
                        mf=sum(t["F"].shape[2] for t in rhs_t),
                        Z=np.ascontiguousarray(np.vstack([t["basis_rom"].T for t in blocks])),
                        Zf=np.ascontiguousarray(np.vstack([t["basis_rom"].T for t in rhs_t])) if rhs_t else None,
                        F_mass=np.ascontiguousarray(mass["F"]), F_lin=cat(lin_t), F_rhs=cat(rhs_t),
                        W=None if nl_t is None else np.ascontiguousarray(nl_t["W"]),
                        C=None if nl_t is None else nl_t["C"], S=None if nl_t is None else nl_t["S"],
                        terms=(mass, lin_t, nl_t, rhs_t))
    c.depth = c.mm + c.ml + c.mn
    return c


def _h_assemble(c, s, un, unm1, T, absolute, fault):
    a = np.abs if absolute else (lambda x: x)
    cast = lambda x: a(np.asarray(x, dtype=T))
    B, r, mm, ml, mn, dt = c.n_mu, c.r, c.mm, c.ml, c.mn, T(c.dt)
    nxt = min(s + 1, c.nt - 1)
    row = lambda tab, name: tab[nxt if fault == "row_" + name else s]
    pts = lambda tab: tab[np.r_[1, 0, 2:B]] if (fault == "swap_points" and B > 1) else tab
    bdf = T(1.5) if (c.bdf2 and s >= 1 and fault != "bdf1") else T(1.0)
    un, unm1 = cast(un), cast(unm1)
    if c.bdf2:
        ustar = 2 * un + unm1 if absolute else (un if fault == "ustar" else 2 * un - unm1)
        past = 2 * un + unm1 / 2 if absolute else 2 * un - unm1 / 2
    else:
        ustar = past = un
    Z = cast(c.Z)
    if fault == "Z_T":
        Z = np.ascontiguousarray(Z.reshape(-1, r, r).transpose(0, 2, 1)).reshape(-1, r * r)
    MN = (pts(cast(row(c.F_mass, "F_mass"))) @ Z[:mm]).reshape(B, r, r)
    K = bdf * MN
    if ml:
        K = K + dt * (pts(cast(row(c.F_lin, "F_lin"))) @ Z[mm:mm + ml]).reshape(B, r, r)
    if mn:
        g = ustar @ cast(c.W).T
        if c.C is not None and fault != "drop_C":
            g = g + pts(cast(row(c.C, "C_nl")))
        if c.S is not None and fault != "drop_S":
            g = pts(cast(row(c.S, "S_nl")))[:, None] * g
        K = K + dt * (g @ Z[mm + ml:]).reshape(B, r, r)
    Mb = MN
    if fault == "prev_MN" and s >= 1:
        Mb = (cast(c.F_mass[s - 1]) @ Z[:mm]).reshape(B, r, r)
    b = np.einsum("bij,bj->bi", Mb, past)
    if c.mf:
        b = b + dt * (pts(cast(row(c.F_rhs, "F_rhs"))) @ cast(c.Zf))
    return K, b


# ---- direct-sweep models -------------------------------------------------------------------------------------------------
def direct_case(seed, N, r, bdf2, pattern="penta", nt=4, n_mu=3, n_terms=3, tril=True, n_rhs=1, dt=0.05):
    """A direct-sweep model on an arbitrary pattern.  Mass: 4 on the diagonal, off-diagonals uniform in [-1, 1] divided
    by twice the larger of the row's and the column's entry count (row and column dominant: the symmetric part is
    positive definite).  Terms and tril: standard normal values on the pattern.  V: a QR factor.  Coefficients: smooth
    in the step with a random offset per point.  Every row with entries gets its diagonal; the rows that
    ``empty_rows`` empties stay empty - they are what that pattern is for (sweep_rows_kernel and the row gather on a row
    without entries), and M_N = V^T M V stays well conditioned since V does not live on six rows (asserted with the other
    conditions by tests/test_sweep_truth_cpu.py)."""
    rng = np.random.RandomState(seed)
    A = penta(N, rng) if pattern == "penta" else pattern_matrix(pattern, N, rng)
    keep = np.diff(A.indptr) > 0 if pattern == "empty_rows" else np.ones(N, dtype=bool)
    S = csr_matrix(((A != 0).astype(np.float64) + csr_matrix((keep.astype(np.float64), (np.arange(N), np.arange(N))), shape=(N, N))))
    S.eliminate_zeros()
    S.sum_duplicates()
    S.sort_indices()
    indptr, indices = S.indptr.astype(np.int64), S.indices.astype(np.int64)
    nnz = indices.size
    row_of = np.repeat(np.arange(N), np.diff(indptr))
    rowcnt, colcnt = np.diff(indptr), np.bincount(indices, minlength=N)
    mass = rng.uniform(-1.0, 1.0, nnz) / (2.0 * np.maximum(rowcnt[row_of], colcnt[indices]))
    mass[row_of == indices] = 4.0
    terms = rng.standard_normal((n_terms, nnz)) if n_terms else None
    trilv = rng.standard_normal(nnz) if tril else None
    V, _ = np.linalg.qr(rng.standard_normal((N, r)))
    steps = np.arange(1, nt + 1)[:, None, None]
    smooth = lambda n: (rng.uniform(0.5, 1.5, (1, n_mu, n)) + 0.3 * np.sin(0.7 * steps + np.arange(n)[None, None, :]))
    term_coef = np.ascontiguousarray(smooth(n_terms)) if n_terms else None
    rhs_terms = 5.0 * rng.standard_normal((n_rhs, N)) if n_rhs else None
    rhs_coef = np.ascontiguousarray(smooth(n_rhs)) if n_rhs else None
    c = SimpleNamespace(kind="direct", N=N, r=r, n_mu=n_mu, nt=nt, dt=dt, bdf2=bool(bdf2), nnz=nnz, indptr=indptr, indices=indices,
                        row_of=row_of, V=np.ascontiguousarray(V), mass=mass, n_terms=n_terms, terms=terms, term_coef=term_coef,
                        tril=trilv, n_rhs=n_rhs, rhs_terms=rhs_terms, rhs_coef=rhs_coef, _proj={})
    c.depth = int(rowcnt.max()) + N
    return c


def csr_mm(c, vals, X):
    """A X for the CSR matrix with value vector ``vals`` on the case's pattern, in the dtype of X."""
    out = np.zeros((c.N, X.shape[1]), dtype=X.dtype)
    np.add.at(out, c.row_of, np.asarray(vals, dtype=X.dtype)[:, None] * X[c.indices])
    return out


def _projections(c, T, absolute):
    """V^T A V of every fixed operator from the CSR data, T V and V^T f, once per case, dtype and absolute flag."""
    key = (np.dtype(T).name, absolute)
    if key not in c._proj:
        a = np.abs if absolute else (lambda x: x)
        V = a(np.asarray(c.V, dtype=T))
        proj = lambda vals: V.T @ csr_mm(c, a(np.asarray(vals, dtype=T)), V)
        c._proj[key] = SimpleNamespace(
            V=V, MN=proj(c.mass), AN=np.stack([proj(t) for t in c.terms]) if c.n_terms else None,
            TV=csr_mm(c, a(np.asarray(c.tril, dtype=T)), V) if c.tril is not None else None,
            fN=a(np.asarray(c.rhs_terms, dtype=T)) @ V if c.n_rhs else None)
    return c._proj[key]


def _d_assemble(c, s, un, unm1, T, absolute, fault):
    a = np.abs if absolute else (lambda x: x)
    cast = lambda x: a(np.asarray(x, dtype=T))
    P = _projections(c, T, absolute)
    B, dt = c.n_mu, T(c.dt)
    nxt = min(s + 1, c.nt - 1)
    row = lambda tab, name: tab[nxt if fault == "row_" + name else s]
    pts = lambda tab: tab[np.r_[1, 0, 2:B]] if (fault == "swap_points" and B > 1) else tab
    bdf = T(1.5) if (c.bdf2 and s >= 1 and fault != "bdf1") else T(1.0)
    un, unm1 = cast(un), cast(unm1)
    if c.bdf2:
        ustar = 2 * un + unm1 if absolute else (un if fault == "ustar" else 2 * un - unm1)
        past = 2 * un + unm1 / 2 if absolute else 2 * un - unm1 / 2
    else:
        ustar = past = un
    K = np.repeat((bdf * P.MN)[None], B, axis=0)
    if c.n_terms:
        coef = pts(cast(row(c.term_coef, "term_coef")))
        if fault == "drop_term":
            coef = coef.copy()
            coef[:, -1] = 0
        K = K + dt * np.einsum("bq,qij->bij", coef, P.AN)
    if c.tril is not None:
        uh = ustar @ P.V.T                                   # u* in FOM coordinates, V u_N*
        for b in range(B):
            if fault == "tril_col":                          # diag(u*) applied to the columns of T instead of its rows
                K[b] = K[b] + dt * (P.V.T @ csr_mm(c, cast(c.tril), uh[b][:, None] * P.V))
            else:
                K[b] = K[b] + dt * (P.V.T @ (uh[b][:, None] * P.TV))
    b = past @ P.MN.T
    if c.n_rhs:
        b = b + dt * (pts(cast(row(c.rhs_coef, "rhs_coef"))) @ P.fN)
    return K, b


# ---- the step, the players and the measure --------------------------------------------------------------------------------
def assemble(c, s, un, unm1, T=LD, absolute=False, fault=None):
    """K_N (n_mu x r x r) and b_N (n_mu x r) of step s from the states un = u^n, unm1 = u^{n-1} (n_mu x r), in dtype T.
    ``absolute``: the same assembly on the absolute values of every operand.  ``fault``: a planted fault (float64 player)."""
    return (_h_assemble if c.kind == "hrom" else _d_assemble)(c, s, un, unm1, T, absolute, fault)


def states(c, uN, s):
    """u^n and u^{n-1} of step s from the trajectory itself (zeros before the start)."""
    zero = np.zeros((c.n_mu, c.r))
    return (uN[:, s - 1] if s >= 1 else zero), (uN[:, s - 2] if s >= 2 else zero)


TRAJECTORY_FAULTS = ("stale_prev", "store_prev")


def play(c, fault=None, conds=None):
    """The float64 NumPy sweep (np.linalg.solve), optionally with a planted fault: NumPy playing the device.
    ``conds``: a list that receives cond_2 of every K_N met."""
    uN = np.zeros((c.n_mu, c.nt, c.r))
    for s in range(c.nt):
        un, unm1 = states(c, uN, s)
        if fault == "stale_prev" and s >= 2:                 # u^{n-1} not updated at the last step close
            unm1 = uN[:, s - 3] if s >= 3 else np.zeros_like(un)
        K, b = assemble(c, s, un, unm1, np.float64, fault=None if fault in TRAJECTORY_FAULTS else fault)
        if conds is not None:
            conds.extend(np.linalg.cond(K).tolist())
        uN[:, s] = np.linalg.solve(K, b[..., None])[..., 0]
    if fault == "store_prev" and c.nt >= 2:                  # the last trajectory row stored one step early
        uN[:, c.nt - 2] = uN[:, c.nt - 1]
    return uN


def gauss_solve(K, b):
    """Gaussian elimination with partial pivoting in the dtype of K (long double: LAPACK has none)."""
    A, y = np.array(K), np.array(b)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], y[[k, p]] = A[[p, k]], y[[p, k]]
        l = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= l[:, None] * A[k, k:][None, :]
        y[k + 1:] -= l * y[k]
    x = np.zeros_like(y)
    for k in range(n - 1, -1, -1):
        x[k] = (y[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def play_longdouble(c):
    """The long-double step iterated as a loop of its own (cross-check against the oracle's loop)."""
    uN = np.zeros((c.n_mu, c.nt, c.r), dtype=LD)
    for s in range(c.nt):
        K, b = assemble(c, s, *states(c, uN, s), LD)
        for p in range(c.n_mu):
            uN[p, s] = gauss_solve(K[p], b[p])
    return uN


def measure(c, uN):
    """The one-step defect of every step and point of the trajectory ``uN`` (n_mu x nt x r, float64).  Returns a
    namespace of (n_mu x nt) arrays: ``ratio`` (the trajectory's own), ``ratio_numpy`` (float64 NumPy step from the same
    two states), ``d2`` / ``b2`` (2-norms of the defect and of b_N), ``floor``, and ``entry`` (the row of the largest
    defect)."""
    B, nt, r = c.n_mu, c.nt, c.r
    out = SimpleNamespace(**{k: np.zeros((B, nt)) for k in ("ratio", "ratio_numpy", "d2", "b2", "floor")}, entry=np.zeros((B, nt), dtype=int))
    for s in range(nt):
        un, unm1 = states(c, uN, s)
        K, b = assemble(c, s, un, unm1, LD)
        Ka, ba = assemble(c, s, un, unm1, LD, absolute=True)
        K64, b64 = assemble(c, s, un, unm1, np.float64)
        x_np = np.linalg.solve(K64, b64[..., None])[..., 0]
        for name, x in (("ratio", uN[:, s]), ("ratio_numpy", x_np)):
            x = np.asarray(x, dtype=LD)
            ax = np.abs(x)
            d = np.einsum("bij,bj->bi", K, x) - b
            floor = EPS * (c.depth * np.einsum("bij,bj->bi", Ka, ax) + r * np.einsum("bij,bj->bi", np.abs(K), ax) + ba).max(axis=1)
            tiny = np.finfo(np.float64).tiny
            getattr(out, name)[:, s] = (np.abs(d).max(axis=1) / np.maximum(floor, tiny)).astype(np.float64)
            if name == "ratio":
                out.d2[:, s] = np.sqrt((d * d).sum(axis=1)).astype(np.float64)
                out.b2[:, s] = np.sqrt((b * b).sum(axis=1)).astype(np.float64)
                out.floor[:, s] = floor.astype(np.float64)
                out.entry[:, s] = np.abs(d).argmax(axis=1)
    return out


def worst(m):
    """(worst ratio / max(ratio_numpy, 1), point, step, entry) of a measure."""
    q = m.ratio / np.maximum(m.ratio_numpy, 1.0)
    b, s = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[b, s]), int(b), int(s), int(m.entry[b, s])


# ---- the oracle's view of a direct-sweep model ---------------------------------------------------------------------------
class DirectFom:
    """A direct-sweep case as the duck-typed FOM of ``oracle.rom_solve_nonlinear`` for parameter point ``b``."""

    def __init__(self, c, b):
        self.c, self.b, self.dt, self.nt, self.bdf2 = c, b, c.dt, c.nt, c.bdf2

    def _csr(self, vals):
        c = self.c
        return csr_matrix((np.asarray(vals, dtype=np.float64), c.indices, c.indptr), shape=(c.N, c.N))

    def _step(self, t):
        return int(round(t / self.dt)) - 1

    def assemble_mass(self, mu, t):
        return self._csr(self.c.mass)

    def assemble_stiffness(self, mu, t):
        c = self.c
        return self._csr(c.term_coef[self._step(t), self.b] @ c.terms if c.n_terms else np.zeros(c.nnz))

    def assemble_convection(self, mu, t):
        return self._csr(np.zeros(self.c.nnz))

    assemble_nonlinear_lifting = assemble_convection

    def assemble_trilinear(self, mu, t, u):
        c = self.c
        return self._csr(u[c.row_of] * c.tril if c.tril is not None else np.zeros(c.nnz))

    def assemble_lifting(self, mu, t):
        c = self.c
        return c.rhs_coef[self._step(t), self.b] @ c.rhs_terms if c.n_rhs else np.zeros(c.N)

    def lifting(self, mu, t):
        return np.zeros(self.c.N)


# ---- the cases of tests/test_sweep_truth_gpu.py (each runs under BDF1 and BDF2) ------------------------------------------
def _split(M):
    """m_mass, lin, m_nl with m_mass + m_lin + m_nl = M."""
    if M == 2:
        return dict(m_mass=1, lin=(), m_nl=1)
    q = M // 4
    return dict(m_mass=q, lin=((q, "spd"), (q, "general")), m_nl=M - 3 * q)


_OPTIONAL = dict(nl_none=dict(nl=None), nl_no_C=dict(nl="noC"), nl_no_S=dict(nl="noS"), nl_bare=dict(nl="bare"),
                 lin_none=dict(lin=()), mass_only=dict(lin=(), nl=None), rhs_two=dict(n_rhs=2),
                 lin_three=dict(lin=((3, "spd"), (5, "general"), (2, "general"))))
H_CASES = {}
for _r in (11, 16):
    for _k, _v in _OPTIONAL.items():
        H_CASES[f"{_k}_r{_r}"] = dict(r=_r, **_v)
for _r in (1, 2, 15, 16, 17, 80, 81, 128):
    H_CASES[f"size_r{_r}"] = dict(r=_r)
for _b in (1, 32, 33):
    H_CASES[f"points_{_b}"] = dict(r=16, n_mu=_b)
for _M in (2, 144, 146, 288, 290, 145):
    H_CASES[f"contraction_{_M}"] = dict(r=16, **_split(_M))
for _nt in (1, 2, 3):
    H_CASES[f"horizon_{_nt}"] = dict(r=16, nt=_nt)
H_GRAPH_CASES = {f"r{_r}_nt{_nt}": dict(r=_r, nt=_nt) for _r in (16, 80) for _nt in (3, 2)}
H_GRAPH_CASES.update(nl_none=dict(r=16, nt=3, nl=None), rhs_two=dict(r=16, nt=3, n_rhs=2))
H_GMRES_CASES = dict(nl_none=dict(r=16, nl=None), lin_none=dict(r=16, lin=()), full_r16=dict(r=16), full_r81=dict(r=81))
H_ZERO_CASES = dict(rhs_none=dict(r=16, n_rhs=0))

D_CASES = {}
for _q in (0, 1, 8, 9, 12):
    D_CASES[f"terms_{_q}"] = dict(N=150, r=5, n_terms=_q)
    D_CASES[f"terms_{_q}_table_520x8"] = dict(N=64, r=4, nt=2, n_mu=520, n_terms=_q) if _q == 8 else None
    D_CASES[f"terms_{_q}_table_460x9"] = dict(N=64, r=4, nt=2, n_mu=460, n_terms=_q) if _q == 9 else None
D_CASES = {k: v for k, v in D_CASES.items() if v is not None}
D_CASES.update(tril_none=dict(N=150, r=5, tril=False), terms_none=dict(N=150, r=6, n_terms=0, tril=True),
               rhs_one=dict(N=150, r=5, n_rhs=1), rhs_three=dict(N=150, r=5, n_rhs=3))
for _p in ("penta",) + PATTERNS:
    for _r in (7, 80):
        D_CASES[f"{_p}_r{_r}"] = dict(N=413, r=_r, pattern=_p, n_mu=2 if _r == 80 else 3)
for _r, _N in ((1, 100), (16, 200), (17, 200), (80, 300), (81, 300), (128, 300)):
    D_CASES[f"size_r{_r}"] = dict(N=_N, r=_r, n_mu=2)
D_CASES.update(square_r16=dict(N=16, r=16), N_257=dict(N=257, r=16), N_3_r1=dict(N=3, r=1),
               points_1=dict(N=100, r=8, n_mu=1), points_33=dict(N=100, r=8, n_mu=33),
               horizon_1=dict(N=100, r=8, nt=1), horizon_2=dict(N=100, r=8, nt=2))
for _r in (64, 112):     # the tile layouts of 4 and 7 block rows, with the sweep's own stage table and its banded hint
    D_CASES[f"size_r{_r}"] = dict(N=300, r=_r, n_mu=2)
D_GMRES_CASES = dict(wide_r7=dict(N=413, r=7, pattern="wide"), tril_none=dict(N=150, r=5, tril=False))
D_ZERO_CASES = dict(rhs_none=dict(N=150, r=5, n_rhs=0))


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def build(kind, name, kw, bdf2):
    """The case ``name`` of a table above: the same generator calls on the CPU and on the GPU side."""
    return (hrom_case if kind == "hrom" else direct_case)(seed=_seed(kind + name) + int(bdf2), bdf2=bdf2, **kw)
