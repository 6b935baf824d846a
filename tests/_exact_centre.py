"""Reference centres for the general exact-FTL solver's non-unique minimisers.

include/ocx.h promises, for ocx_exact_ball_solve, the central path's limit where the
minimiser of ½Σ|z_i·x − y_i| over the ball is not unique: the analytic centre of the
optimal face.  Here that centre comes from its DEFINITION on faces known by construction:
maximise the sum of the logs of the slacks that are not identically zero on the face —

  * every row with r_i ≢ 0 on the face gives log|r_i(x)|  (the eliminated-slack barrier of
    ocx_exact_ball.hip: s_i² − r_i² = 2μ s_i with s_i → 2|r_i|),
  * l2 gives log(1 − ‖x‖²), linf gives Σ_j log(1 − x_j²) over the coordinates not fixed at
    ±1, l1 gives the (x, u) terms log(u_j ∓ x_j), log(1 − Σu) that are not identically 0 —

by Newton on the equality-constrained concave problem in float64 (KKT steps; the last step
starts from a Newton decrement below 1e-9 and leaves its square), never by a float64
central path.  `mp_central_path` is the independent cross-check: the documented F_μ itself,
followed in 60-digit arithmetic to μ = 1e-14.

Each case is a function returning a dict: z [T, d], y [T], norm, all_prefixes, `prefixes`
(the prefix lengths checked), `centre` {n: x} and `other` {n: a second point of the same
optimal face}.  numpy / scipy / mpmath only; no GPU."""
import functools

import mpmath as mp
import numpy as np
from scipy.optimize import linprog

from tests._scipy_solvers import lp_solve

# one or more dimensions per kernel and instantiation: registers (d <= 10), LDS (<= 64),
# HBM scratch (Q = 2 to d = 128, Q = 4 to 256)
DIMS = (5, 10, 11, 33, 64, 65, 100, 256)


def tier(d):
    return "reg" if d <= 10 else ("lds" if d <= 64 else ("hbm-q2" if d <= 128 else "hbm-q4"))


def tie_coords(d, k=2):
    """Coordinates for the constructed ties, across the lane and Q boundaries: 0 and d − 1
    (and the middle), 63 and 64 (and 0) where d >= 65."""
    if d >= 65:
        return (63, 64, 0)[:k]
    return (0, d - 1, d // 2)[:k]


# ---------------------------------------------------------------- the definition's solver
def log_centre(C, e, w, v0, A=None, b=None, ball2=None, iters=200):
    """argmax_v Σ_k w_k log(C_k·v + e_k) [+ log(1 − ‖v[:ball2]‖²)]  s.t.  A v = b, from the
    strictly feasible v0 by damped Newton on the KKT system."""
    v = np.array(v0, dtype=np.float64)
    D = v.size
    m = 0 if A is None else A.shape[0]
    for _ in range(iters):
        s = C @ v + e
        assert np.all(s > 0.0)
        g = C.T @ (w / s)
        H = -(C.T * (w / s ** 2)) @ C
        if ball2:
            q = 1.0 - v[:ball2] @ v[:ball2]
            g[:ball2] += -2.0 * v[:ball2] / q
            H[:ball2, :ball2] += -2.0 * np.eye(ball2) / q - 4.0 * np.outer(v[:ball2], v[:ball2]) / q ** 2
        if m:
            K = np.block([[-H, A.T], [A, np.zeros((m, m))]])
            step = np.linalg.solve(K, np.r_[g, b - A @ v])[:D]
        else:
            step = np.linalg.solve(-H, g)
        lam = np.sqrt(max(step @ (-H) @ step, 0.0))
        t = 1.0 if lam <= 0.25 else 1.0 / (1.0 + lam)
        while True:                                   # stay strictly inside the domain
            vn = v + t * step
            ok = np.all(C @ vn + e > 0.0)
            if ball2:
                ok = ok and vn[:ball2] @ vn[:ball2] < 1.0
            if ok:
                break
            t *= 0.5
        v = vn
        if lam < 1e-9:                                # quadratic: this step left ~lam² of error
            return v
    raise AssertionError("log_centre did not converge")


def l1_axis_centre(z, y):
    """Rows c_i·e_{j_i} (0 < c_i <= 1) with y = +1: ½Σ|r| = ½(n − S·x) on the ball, so the
    optimal face is the simplex over the coordinates M at max S_j.  On it u = x, so the terms
    left are log(1 − c_i x_{j_i}) per row in M and log(u_j + x_j) = log 2x_j per j in M.
    Returns (centre, M) or (None, M) where the maximum is unique."""
    n, d = z.shape
    assert np.all(y == 1.0) and np.all((z != 0.0).sum(axis=1) == 1) and z.min() >= 0.0 and z.max() <= 1.0
    S = z.sum(axis=0)
    M = np.flatnonzero(S == S.max())
    if M.size < 2:
        return None, M
    rows = [i for i in range(n) if z[i, M].any()]
    C = np.vstack([-z[rows][:, M], np.eye(M.size)])
    e = np.r_[np.ones(len(rows)), np.zeros(M.size)]
    v = log_centre(C, e, np.ones(C.shape[0]), np.full(M.size, 1.0 / M.size),
                   A=np.ones((1, M.size)), b=np.ones(1))
    x = np.zeros(d)
    x[M] = v
    return x, M


def linf_sign_centre(z, y):
    """y = ±1 rows whose residuals keep their sign on the face: ½Σ|r| = ½(n − S·x), S = Σ y z,
    so x_j = sign(S_j) where S_j != 0 and x_j is free where S_j = 0 exactly.  The terms left
    are log(1 − y_i z_i·x) per row and log(1 − x_j²) per free coordinate (an untouched free
    coordinate has only the latter: centre 0).  A residual that would change sign inside the
    box is a wall of the face, which its own log keeps the centre from.  Returns
    (centre, free touched coordinates)."""
    n, d = z.shape
    assert np.all(np.abs(y) == 1.0)
    S = (y[:, None] * z).sum(axis=0)
    x = np.sign(S)
    F = np.flatnonzero((S == 0.0) & (z != 0.0).any(axis=0))
    if F.size == 0:
        return x, F
    C = np.vstack([-(y[:, None] * z[:, F]), -np.eye(F.size), np.eye(F.size)])
    e = np.r_[1.0 - y * (z @ x), np.ones(2 * F.size)]
    x[F] = log_centre(C, e, np.ones(C.shape[0]), np.zeros(F.size))
    return x, F


def interp_centre(Z, y, norm):
    """The face {Zx = y} ∩ ball (every residual ≡ 0): only the ball's terms remain.  l2: the
    min-norm interpolant pinv(Z) y; linf: argmax Σ log(1 − x_j²); l1: argmax over (x, u) of
    Σ log(u_j − x_j) + Σ log(u_j + x_j) + log(1 − Σu).  None where the min-l2-norm
    interpolant is not well inside the ball (no strictly feasible start from it)."""
    n, d = Z.shape
    x0 = np.linalg.pinv(Z) @ y
    if norm == "l2":
        return x0 if np.linalg.norm(x0) < 1.0 else None
    I = np.eye(d)
    if norm == "linf":
        if np.abs(x0).max() > 0.95:
            return None
        return log_centre(np.vstack([-I, I]), np.ones(2 * d), np.ones(2 * d), x0, A=Z, b=y)
    if np.abs(x0).sum() > 0.95:
        return None
    u0 = np.abs(x0) + (1.0 - np.abs(x0).sum()) / (2.0 * d)
    C = np.vstack([np.hstack([-I, I]), np.hstack([I, I]), np.r_[np.zeros(d), -np.ones(d)][None]])
    e = np.r_[np.zeros(2 * d), 1.0]
    v = log_centre(C, e, np.ones(2 * d + 1), np.r_[x0, u0], A=np.hstack([Z, np.zeros((n, d))]), b=y)
    return v[:d]


def ball_norm(x, norm):
    return {"l2": np.linalg.norm(x), "l1": np.abs(x).sum(), "linf": np.abs(x).max()}[norm]


def face_far_point(Z, y, norm, centre):
    """A second point of the interpolation face far from the centre: under l2 a null-space
    step to norm 0.99; under linf / l1 the face's extreme point along the coordinate the
    null space moves most (an LP)."""
    n, d = Z.shape
    P = np.eye(d) - np.linalg.pinv(Z) @ Z                 # projector on null(Z)
    j = int(np.argmax(np.diag(P)))
    if norm == "l2":
        v = P[:, j] / np.linalg.norm(P[:, j])
        return centre + np.sqrt(0.99 ** 2 - centre @ centre) * v
    c = np.zeros(2 * d)
    c[j], c[d + j] = -1.0, 1.0                            # max x_j, x = p − q, p, q >= 0
    if norm == "linf":
        res = linprog(c, A_eq=np.hstack([Z, -Z]), b_eq=y, bounds=[(0, 1)] * (2 * d), method="highs")
    else:
        res = linprog(c, A_eq=np.hstack([Z, -Z]), b_eq=y, A_ub=np.ones((1, 2 * d)), b_ub=[1.0],
                      bounds=[(0, None)] * (2 * d), method="highs")
    assert res.status == 0
    x = res.x[:d] - res.x[d:]
    x -= np.linalg.pinv(Z) @ (Z @ x - y)                  # HiGHS's 1e-9 off the face, removed
    return centre + 0.999 * (x - centre)                  # strictly inside the ball


# ---------------------------------------------------------------- the 60-digit cross-check
def mp_central_path(z, y, norm, mu_end="1e-14", dps=60):
    """The documented F_μ (ocx_exact_ball.hip's header) followed by damped Newton in
    `dps`-digit arithmetic from μ = 1 to mu_end (μ /= 10 once the decrement is below 1/4,
    1e-25 at the last level); (x, u) under l1.  Small problems only (d <= 8)."""
    with mp.workdps(dps):
        n, d = z.shape
        Zm = [[mp.mpf(float(z[i, j])) for j in range(d)] for i in range(n)]
        ym = [mp.mpf(float(v)) for v in y]
        D = 2 * d if norm == "l1" else d
        v = [mp.mpf(0)] * d + ([mp.mpf(1) / (2 * d)] * d if norm == "l1" else [])
        mu, mu_end = mp.mpf(1), mp.mpf(mu_end)

        def in_domain(v):
            if norm == "l2":
                return sum(t * t for t in v) < 1
            if norm == "linf":
                return all(abs(t) < 1 for t in v)
            return all(abs(v[j]) < v[d + j] for j in range(d)) and sum(v[d:]) < 1

        for _ in range(4000):
            g = [mp.mpf(0)] * D
            H = mp.zeros(D, D)
            for i in range(n):
                r = sum(Zm[i][j] * v[j] for j in range(d)) - ym[i]
                rt = mp.sqrt(mu * mu + r * r)
                s = mu + rt
                g1, h1 = r / (mu * s), 1 / (s * rt)
                for j in range(d):
                    if Zm[i][j] == 0:
                        continue
                    g[j] += g1 * Zm[i][j]
                    for k in range(d):
                        H[j, k] += h1 * Zm[i][j] * Zm[i][k]
            if norm == "l2":
                q = 1 - sum(t * t for t in v)
                for j in range(d):
                    g[j] += 2 * v[j] / q
                    H[j, j] += 2 / q
                    for k in range(d):
                        H[j, k] += 4 * v[j] * v[k] / (q * q)
            elif norm == "linf":
                for j in range(d):
                    g[j] += 1 / (1 - v[j]) - 1 / (1 + v[j])
                    H[j, j] += 1 / (1 - v[j]) ** 2 + 1 / (1 + v[j]) ** 2
            else:
                w = 1 - sum(v[d:])
                for j in range(d):
                    a, c = v[d + j] - v[j], v[d + j] + v[j]
                    g[j] += 1 / a - 1 / c
                    g[d + j] += -1 / a - 1 / c + 1 / w
                    H[j, j] += 1 / a ** 2 + 1 / c ** 2
                    H[d + j, d + j] += 1 / a ** 2 + 1 / c ** 2
                    H[j, d + j] += -1 / a ** 2 + 1 / c ** 2
                    H[d + j, j] += -1 / a ** 2 + 1 / c ** 2
                    for k in range(d):
                        H[d + j, d + k] += 1 / w ** 2
            step = mp.lu_solve(H, mp.matrix([-t for t in g]))
            lam = mp.sqrt(-sum(step[j] * g[j] for j in range(D)))
            t = mp.mpf(1) if lam <= mp.mpf("0.25") else 1 / (1 + lam)
            while True:
                vn = [v[j] + t * step[j] for j in range(D)]
                if in_domain(vn):
                    break
                t /= 2
            v = vn
            if mu > mu_end * mp.mpf("1.5"):
                if lam < mp.mpf("0.25"):
                    mu /= 10
            elif lam < mp.mpf("1e-25"):
                return np.array([float(t) for t in v[:d]])
        raise AssertionError("mp_central_path did not converge")


# ---------------------------------------------------------------- the cases
def _case(z, y, norm, prefixes, centre, other, *, family, all_prefixes=True, tied=None):
    return {"z": z, "y": y, "norm": norm, "d": z.shape[1], "family": family,
            "all_prefixes": all_prefixes, "prefixes": list(prefixes), "centre": centre,
            "other": other, "tied": tied}


def _l1_axis_case(z, family, prefixes=None):
    T, d = z.shape
    y = np.ones(T)
    centre, other = {}, {}
    for n in range(1, T + 1):
        c, M = l1_axis_centre(z[:n], y[:n])
        if c is not None:
            centre[n] = c
            other[n] = np.zeros(d)
            other[n][M[0]] = 1.0                       # the closed form: the first largest |S_j|
    tied = sorted(centre)
    return _case(z, y, "l1", prefixes if prefixes is not None else tied, centre, other,
                 family=family, tied=tied)


@functools.lru_cache(maxsize=None)
def l1_tie_symmetric(d):
    """Rows alternating e_p, e_q with y = +1: tied at every even prefix, centre ½(e_p + e_q)."""
    p, q = tie_coords(d)
    z = np.zeros((14, d))
    z[0::2, p] = 1.0
    z[1::2, q] = 1.0
    return _l1_axis_case(z, "l1-tie-sym")


@functools.lru_cache(maxsize=None)
def l1_tie_asymmetric(d, a=4):
    """a rows 1.0·e_p, then 2a rows 0.5·e_q, y = +1: tied at n = 3a only, where the centre
    maximises a·log(1 − x_p) + 2a·log(1 − ½x_q) + log x_p + log x_q on x_p + x_q = 1
    (a = 4: x_p = 0.3950806…)."""
    p, q = tie_coords(d)
    z = np.zeros((3 * a, d))
    z[:a, p] = 1.0
    z[a:, q] = 0.5
    return _l1_axis_case(z, "l1-tie-asym")


@functools.lru_cache(maxsize=None)
def l1_tie_threeway(d, a=3):
    """a rows e_p, a rows e_q, 2a rows ½e_r: e_p and e_q stay tied from n = 2a on, and all three
    coordinates tie at n = 4a."""
    p, q, r = tie_coords(d, 3)
    z = np.zeros((4 * a, d))
    z[:a, p] = 1.0
    z[a:2 * a, q] = 1.0
    z[2 * a:, r] = 0.5
    c = _l1_axis_case(z, "l1-tie-3way")
    assert c["tied"] == list(range(2 * a, 4 * a + 1))
    return c


def _linf_case(z, y, family, prefixes):
    T, d = z.shape
    centre, other, tied = {}, {}, []
    for n in range(1, T + 1):
        c, F = linf_sign_centre(z[:n], y[:n])
        S = (y[:n, None] * z[:n]).sum(axis=0)
        if np.any((S == 0.0) & (z[:n] != 0.0).any(axis=0)):
            tied.append(n)
        if n in prefixes:
            centre[n] = c
            other[n] = c.copy()
            other[n][F[0]] = 1.0                       # a vertex of the face
    return _case(z, y, "linf", prefixes, centre, other, family=family, tied=tied)


@functools.lru_cache(maxsize=None)
def linf_tie_asymmetric(d, a=4):
    """A touched coordinate p with S_p = 0 beside a coordinate q with S_q != 0 that shifts
    the two row groups' residuals unequally: a rows (½, 0.1) with y = +1, then 2a rows
    (¼, 0.3) with y = −1.  S_p = 0 at n = 3a, S_q < 0 so x_q = −1, and the centre maximises
    a·log(1.1 − ½x) + 2a·log(0.7 + ¼x) + log(1 − x²) over x = x_p: off 0."""
    p, q = tie_coords(d)
    z = np.zeros((3 * a, d))
    y = np.ones(3 * a)
    z[:a, p], z[:a, q] = 0.5, 0.1
    z[a:, p], z[a:, q] = 0.25, 0.3
    y[a:] = -1.0
    return _linf_case(z, y, "linf-tie-asym", [3 * a])


@functools.lru_cache(maxsize=None)
def linf_tie_wall(d, a=4):
    """The same with rows outside the closed form's regime (‖z‖₁ > 1): a rows (1, 0.2) with
    y = +1, 2a rows (½, 0.6) with y = −1.  x_q = −1, the residuals on the face are x − 1.2
    and ½x + 0.4, and the second changes sign at x = −0.8: the optimal face is
    x_p ∈ [−0.8, 1], walled by that row's own log."""
    p, q = tie_coords(d)
    z = np.zeros((3 * a, d))
    y = np.ones(3 * a)
    z[:a, p], z[:a, q] = 1.0, 0.2
    z[a:, p], z[a:, q] = 0.5, 0.6
    y[a:] = -1.0
    return _linf_case(z, y, "linf-tie-wall", [3 * a])


@functools.lru_cache(maxsize=None)
def linf_tie_symmetric(d):
    """½e_p rows with alternating labels: S_p returns to 0 at every even prefix with
    symmetric residuals, so the centre is exactly 0 — as the closed form's answer, while a
    simplex solver returns a vertex."""
    p = tie_coords(d)[1]
    z = np.zeros((14, d))
    y = np.ones(14)
    z[:, p] = 0.5
    y[1::2] = -1.0
    return _linf_case(z, y, "linf-tie-sym", list(range(2, 15, 2)))


@functools.lru_cache(maxsize=None)
def l1_near_bound(d, eta=4e-4):
    """A centre coordinate inside the polish's coarsest kZero (1e-3).  Counts alone cannot put
    it there: on an axis-aligned tie the rows' net pull on x_p at x_p = 0 is S·c_q/(1 − c_q)
    >= 0, so x_p >= 1/(1 + S) needs thousands of rows.  Instead the face itself is short:
    4 rows e_p and 5 rows e_q (y = +1) prefer e_q by slope ½, and one row e_p with label η
    pays that slope back on x_p ∈ [0, η].  The optimal face is {x_p ∈ [0, η], x_q = 1 − x_p}
    and its centre maximises 5·log(1 − x_p) + 6·log x_p + log(η − x_p): x_p ≈ 6η/7."""
    p, q = tie_coords(d)
    z = np.zeros((10, d))
    y = np.ones(10)
    z[:4, p] = 1.0
    z[4:9, q] = 1.0
    z[9, p], y[9] = 1.0, eta
    C = np.array([[-1.0], [1.0], [-1.0]])
    xp = log_centre(C, np.array([1.0, 0.0, eta]), np.array([5.0, 6.0, 1.0]), np.array([eta / 2]))[0]
    c = np.zeros(d)
    c[p], c[q] = xp, 1.0 - xp
    o = np.zeros(d)
    o[q] = 1.0
    return _case(z, y, "l1", [10], {10: c}, {10: o}, family="l1-near-bound")


def _linf_near_q(a, x):
    """The second group's q-entry that puts the asymmetric linf centre at x_p = x: with
    x_q = +1 the centre maximises a·log(0.9 − ½x) + 2a·log(1 + Q + ¼x) + log(1 − x²), whose
    stationarity gives Q in closed form."""
    return 0.5 * a / (0.5 * a / (0.9 - 0.5 * x) + 2.0 * x / (1.0 - x * x)) - 1.0 - 0.25 * x


@functools.lru_cache(maxsize=None)
def linf_near_bound(d, a=4):
    """The asymmetric linf construction with the second group's shift tuned so that the free
    coordinate of the centre is 3e-4."""
    p, q = tie_coords(d)
    z = np.zeros((3 * a, d))
    y = np.ones(3 * a)
    z[:a, p], z[:a, q] = 0.5, 0.1
    z[a:, p], z[a:, q] = 0.25, _linf_near_q(a, 3e-4)
    y[a:] = -1.0
    return _linf_case(z, y, "linf-near-bound", [3 * a])


INTERP_SCALE = {"l2": 0.4, "linf": 0.4, "l1": 0.4}     # l1: divided by sqrt(d)


@functools.lru_cache(maxsize=None)
def interpolation(norm, d):
    """n < d rows N(0,1) with y = c·N(0,1): the optimum is 0 on {Zx = y} ∩ ball.  T = d + 8
    rows over all prefixes (T = 16 at d = 256); a prefix is checked when n < d and the
    centre's norm is <= 0.9 and the face holds a point >= 0.1 (∞-norm) from the centre."""
    T = d + 8 if d < 256 else 16
    rng = np.random.default_rng(7000 + d)
    z = rng.standard_normal((T, d))
    c = INTERP_SCALE[norm] / (np.sqrt(d) if norm == "l1" else 1.0)
    y = c * rng.standard_normal(T)
    centre, other = {}, {}
    for n in range(1, min(T, d - 1) + 1):
        x = interp_centre(z[:n], y[:n], norm)
        if x is not None and ball_norm(x, norm) <= 0.9:
            far = face_far_point(z[:n], y[:n], norm, x)
            # an l1 face narrows in the ∞-norm as n grows (a null vector of n generic rows has
            # n + 1 or more nonzeros sharing an l1 budget below 1): a prefix is checked only
            # where a second point of the face lies >= 0.1 away, so that the bar stays sharp
            if np.abs(far - x).max() >= 0.1:
                centre[n] = x
                other[n] = far
    case = _case(z, y, norm, sorted(centre), centre, other, family="interp")
    case["eligible"] = min(T, d - 1)
    return case


@functools.lru_cache(maxsize=None)
def unique_vertex(norm, d):
    """Generic n >= d clipped rows with ±1 labels: the LP minimiser is a unique vertex (HiGHS),
    and the path's limit is that vertex."""
    T = d + 55
    rng = np.random.default_rng(3 + d)
    z = rng.standard_normal((T, d))
    z /= np.maximum(1.0, np.linalg.norm(z, axis=1, keepdims=True))
    y = np.where(rng.random(T) < 0.5, -1.0, 1.0)
    x, _ = lp_solve(z, y, norm)
    return _case(z, y, norm, [T], {T: x}, {}, family="vertex", all_prefixes=False)


NONUNIQUE = {
    "l1-tie-sym": l1_tie_symmetric, "l1-tie-asym": l1_tie_asymmetric, "l1-tie-3way": l1_tie_threeway,
    "linf-tie-asym": linf_tie_asymmetric, "linf-tie-wall": linf_tie_wall,
    "linf-tie-sym": linf_tie_symmetric, "l1-near-bound": l1_near_bound,
    "linf-near-bound": linf_near_bound,
    "interp-l2": functools.partial(interpolation, "l2"),
    "interp-linf": functools.partial(interpolation, "linf"),
    "interp-l1": functools.partial(interpolation, "l1"),
}
TIE_FAMILIES = ("l1-tie-sym", "l1-tie-asym", "l1-tie-3way", "linf-tie-asym", "linf-tie-wall",
                "linf-tie-sym", "linf-near-bound")
NEAR_BOUND = ("l1-near-bound", "linf-near-bound")
