"""CPU references of SuperGlue's optimal-matching layer, written from the published algorithm
(Sarlin et al., CVPR 2020, section 3.2 and the authors' log_optimal_transport): the reference project's tree holds only the
call into a TorchScript file it does not ship.

    assign          float64 numpy, the dustbin row and column implicit (one extra term per logsumexp): THE reference
    assign_bordered float64 numpy on the materialised (m + 1) x (n + 1) matrix: the published form, checks the former
    assign_torch32  fp32 with torch.logsumexp on the CPU on the bordered matrix: what the network's forward would run
    select          argmax (lowest index on ties), mutual check, scores, the two thresholds
    cases           the planted pairs the tests and the golden file share
"""
import numpy as np


def scores(d0, d1):
    """S = d0 d1^T / sqrt(D) in float64; d0 [m][D], d1 [n][D]."""
    return d0.astype(np.float64) @ d1.astype(np.float64).T / np.sqrt(float(d0.shape[1]))


def _lse(x, axis):
    mx = x.max(axis=axis, keepdims=True)
    return (mx + np.log(np.exp(x - mx).sum(axis=axis, keepdims=True))).squeeze(axis)


def marginals(m, n):
    norm = -np.log(float(m + n))
    log_mu = np.full(m + 1, norm)
    log_nu = np.full(n + 1, norm)
    log_mu[m] = np.log(float(n)) + norm
    log_nu[n] = np.log(float(m)) + norm
    return norm, log_mu, log_nu


def assign(S, alpha=1.0, iterations=100):
    """logP [m + 1][n + 1] (dustbins last), u, v in float64; the bordered matrix is never built."""
    S = np.asarray(S, np.float64)
    m, n = S.shape
    norm, log_mu, log_nu = marginals(m, n)
    u, v = np.zeros(m + 1), np.zeros(n + 1)
    for _ in range(iterations):
        inner = _lse(np.concatenate([S + v[None, :n], np.full((m, 1), alpha + v[n])], axis=1), 1)
        dust = _lse(alpha + v, 0)
        u = log_mu - np.append(inner, dust)
        inner = _lse(np.concatenate([S + u[:m, None], np.full((1, n), alpha + u[m])], axis=0), 0)
        dust = _lse(alpha + u, 0)
        v = log_nu - np.append(inner, dust)
    Z = np.full((m + 1, n + 1), float(alpha))
    Z[:m, :n] = S
    return Z + u[:, None] + v[None, :] - norm, u, v


def assign_bordered(S, alpha=1.0, iterations=100):
    S = np.asarray(S, np.float64)
    m, n = S.shape
    norm, log_mu, log_nu = marginals(m, n)
    Z = np.full((m + 1, n + 1), float(alpha))
    Z[:m, :n] = S
    u, v = np.zeros(m + 1), np.zeros(n + 1)
    for _ in range(iterations):
        u = log_mu - _lse(Z + v[None, :], 1)
        v = log_nu - _lse(Z + u[:, None], 0)
    return Z + u[:, None] + v[None, :] - norm


def assign_torch32(S, alpha=1.0, iterations=100):
    """The published implementation, fp32 on the CPU: torch.logsumexp over the bordered matrix."""
    import torch
    S = torch.as_tensor(np.asarray(S, np.float32))
    m, n = S.shape
    a = torch.tensor(float(alpha), dtype=torch.float32)
    Z = torch.cat([torch.cat([S, a.expand(m, 1)], 1), a.expand(1, n + 1)], 0)
    ms, ns = torch.tensor(float(m)), torch.tensor(float(n))
    norm = -(ms + ns).log()
    log_mu = torch.cat([norm.expand(m), ns.log()[None] + norm])
    log_nu = torch.cat([norm.expand(n), ms.log()[None] + norm])
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iterations):
        u = log_mu - torch.logsumexp(Z + v[None, :], dim=1)
        v = log_nu - torch.logsumexp(Z + u[:, None], dim=0)
    return (Z + u[:, None] + v[None, :] - norm).numpy()


def select(logP, match_threshold=0.2, score_threshold=0.5):
    """From logP [m + 1][n + 1]: matches0, matches1, mscores0, mscores1, table (both thresholds).  np.argmax takes the lowest
    index on ties."""
    inner = logP[:-1, :-1]
    m, n = inner.shape
    i0, i1 = inner.argmax(1), inner.argmax(0)
    mutual0 = i1[i0] == np.arange(m)
    mutual1 = i0[i1] == np.arange(n)
    ms0 = np.where(mutual0, np.exp(inner.max(1)), 0.0)
    ms1 = np.where(mutual1, ms0[i1], 0.0)
    m0 = np.where(mutual0 & (ms0 > match_threshold), i0, -1)
    m1 = np.where(mutual1 & (ms1 > match_threshold), i1, -1)
    table = np.where((m0 >= 0) & (ms0 > score_threshold), m0, -1)
    return dict(matches0=m0, matches1=m1, mscores0=ms0, mscores1=ms1, table=table)


def undecided(logP, tol, match_threshold=0.2, score_threshold=0.5):
    """Rows and columns an implementation within `tol` of logP may decide otherwise: the top-two margin of the row, or of
    its best column, is below 2 tol, or the score is within tol of a threshold.  Returns (rows [m] bool, cols [n] bool)."""
    inner = logP[:-1, :-1]
    m, n = inner.shape

    def margin(a):          # top-two margin along the last axis (one entry: infinite)
        if a.shape[1] < 2:
            return np.full(a.shape[0], np.inf)
        p = np.partition(a, a.shape[1] - 2, axis=1)
        return p[:, -1] - p[:, -2]

    rm, cm = margin(inner), margin(inner.T)
    i0, i1 = inner.argmax(1), inner.argmax(0)
    s0, s1 = np.exp(inner.max(1)), np.exp(inner.max(0))
    near = lambda s: (np.abs(s - match_threshold) <= tol) | (np.abs(s - score_threshold) <= tol)
    rows = (rm < 2 * tol) | (cm[i0] < 2 * tol) | near(s0)
    cols = (cm < 2 * tol) | (rm[i1] < 2 * tol) | near(s1)
    return rows, cols


# ---- the cases the CPU test, the GPU test and the golden file share ---------------------------------------------------------

SHAPES = [(1, 1), (1, 5), (7, 3), (33, 47), (64, 64), (200, 257), (5, 2100), (2100, 5)]
RAGGED = [(200, 257), (0, 40), (33, 47), (272, 272)]          # one batch in M = N = 272
D = 256


def planted_case(m, n, seed, D=D):
    """Planted matches plus noise: about 60 % of the smaller side planted; gain as reconstructor_amd.superglue.planted_pair."""
    from reconstructor_amd.superglue import planted_pair
    rng = np.random.default_rng(seed)
    k = int(round(0.6 * min(m, n)))
    return planted_pair(rng, m, n, k, D=D)


def case_seed(m, n):
    return 1000 * m + n
