"""Reference for "distinct alternatives" (include/gpmp2mi.h): trajectory distances in np.longdouble and in plain float64,
and the leader rule as a literal loop.  Written from the definitions in the header, independently of
gpmp2_amd.scoring.group_rule, so that the two can be compared.  Also the inputs the tests share."""
import numpy as np

MAX_STATE, RMS = 0, 1


def distances(traj, D, weights=None, metric=MAX_STATE, dtype=np.longdouble):
    """dist [B][B] between the configuration halves of traj [B][N+1][2D], evaluated in `dtype`."""
    x = np.asarray(traj)[:, :, :D].astype(dtype)
    B, S = x.shape[0], x.shape[1]
    w = np.ones(D, dtype=dtype) if weights is None else np.asarray(weights).astype(dtype)
    out = np.zeros((B, B), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            diff = x[b][None] - x                      # [B][S][D]
            s = np.zeros((B, S), dtype=dtype)
            for d in range(D):                         # ascending d
                s = s + w[d] * (diff[:, :, d] * diff[:, :, d])
            if metric == MAX_STATE:
                m = s.max(axis=1)
                m = np.where(np.isnan(s).any(axis=1), np.nan, m)
            else:
                m = np.zeros(B, dtype=dtype)
                for i in range(S):                     # ascending i
                    m = m + s[:, i]
                m = m / dtype(S)
            out[b] = np.sqrt(m)
    return out


def rule(dist, score, eligible, radius):
    """The leader rule, literally: (mode [B], leaders [B], sizes [B], n_modes)."""
    B = len(score)
    mode, leaders, sizes = [-1] * B, [], []
    takes_part = [b for b in range(B) if (eligible is None or eligible[b] != 0) and np.isfinite(score[b])]
    for b in sorted(takes_part, key=lambda r: (score[r], r)):
        for k, leader in enumerate(leaders):
            if dist[b][leader] <= radius:              # False for NaN
                mode[b] = k
                sizes[k] += 1
                break
        else:
            mode[b] = len(leaders)
            leaders.append(b)
            sizes.append(1)
    n = len(leaders)
    return (np.array(mode, dtype=np.int32), np.array(leaders + [-1] * (B - n), dtype=np.int32),
            np.array(sizes + [0] * (B - n), dtype=np.int32), n)


def gap_radius(dist_ref, rows=None):
    """The geometric mean of the two sides of the largest gap between the sorted positive finite reference distances
    (of `rows` only, if given).  Asserts that no reference distance lies within 1e-9 * radius of it: a condition on the
    inputs, after which `dist <= radius` is the same statement for the reference and for a float64 evaluation."""
    d = np.asarray(dist_ref, dtype=np.longdouble)
    if rows is not None:
        d = d[np.ix_(rows, rows)]
    v = np.unique(d[np.triu_indices(d.shape[0], 1)])
    v = v[np.isfinite(v) & (v > 0)]
    assert v.size >= 2, "not enough distinct distances for a gap"
    i = int(np.argmax(np.diff(v)))
    radius = float(np.sqrt(v[i] * v[i + 1]))
    finite = np.asarray(dist_ref, dtype=np.longdouble)
    finite = finite[np.isfinite(finite)]
    assert (np.abs(finite - radius) > 1e-9 * radius).all(), "a reference distance sits on the radius"
    return radius


def bound(d_ref, D, N, metric):
    """|d - d_ref| <= (n + 5) 2^-52 d_ref, n = D for MAX_STATE and D (N+1) for RMS (derivation: tests/test_gpu_group.py)."""
    n = D if metric == MAX_STATE else D * (N + 1)
    return (n + 5) * 2.0 ** -52 * np.asarray(d_ref, dtype=np.longdouble)


def random_traj(rng, B, N, D, scale=1.0):
    return rng.standard_normal((B, N + 1, 2 * D)) * scale


def synthetic_modes(rng, G, B, N, D, delta=1e-3):
    """B rows around G <= D smooth centre trajectories: a centre plus noise whose norm per state is <= delta.  Centre g
    is 2 e_g plus a smooth wiggle of at most 0.1 per coordinate, so in both metrics every pair of centres is
    2 sqrt(2) +- 0.2 sqrt(D) apart: for D <= 7 a band narrower than its lower edge, and the largest gap between the
    sorted distances is the one between "same centre" (<= 2 delta) and "different centres".
    Returns (traj [B][N+1][2D], centre index [B])."""
    assert G <= D <= 7
    t = np.linspace(0.0, 1.0, N + 1)[:, None]
    centres = np.zeros((G, N + 1, 2 * D))
    for g in range(G):
        a, b = rng.uniform(-1, 1, D), rng.uniform(-1, 1, D)
        centres[g, :, :D] = 0.05 * (a * t + b * np.sin(np.pi * t))
        centres[g, :, g] += 2.0
        centres[g, :, D:] = rng.standard_normal((N + 1, D))
    which = rng.integers(0, G, size=B)
    which[:min(G, B)] = np.arange(min(G, B))                            # every centre has a row
    noise = rng.standard_normal((B, N + 1, D))
    noise *= delta * rng.uniform(0.1, 1.0, (B, N + 1, 1)) / np.linalg.norm(noise, axis=2, keepdims=True)
    traj = centres[which].copy()
    traj[:, :, :D] += noise
    return traj, which


def scores_with_ties(rng, B, p_ineligible=0.15):
    """scores from a small set (many exact ties), a few non-finite; eligible int32 [B] with some zeros"""
    values = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, np.nan, np.inf])
    p = np.array([0.14] * 7 + [0.01, 0.01])
    score = rng.choice(values, size=B, p=p / p.sum()) + rng.integers(0, 3, size=B) * 0.25
    eligible = (rng.uniform(size=B) >= p_ineligible).astype(np.int32)
    return score, eligible
