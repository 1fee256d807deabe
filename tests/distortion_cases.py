"""Inputs and the float64 truth of the distortion-loss tests (tests/test_distortion.py, tests/test_guard_bands_distortion.py,
tests/golden/make_golden_distortion.py).  Plain helper module (like helpers.py): numpy only, nothing here touches a device.

rows(kind, R, N, seed) -> (t [R, N+1], w [R, N]) float32, t nondecreasing on [0, 1] with t[0] = 0 and t[-1] = 1 (except
'tiny'), w non-negative:
  random     softmax weights on sorted uniform knots
  plateau    the same with a run of three equal knots t_k = t_{k+1} = t_{k+2} per row (two where N = 1: an empty interval)
  zero       all-zero weights
  onehot     one weight of 1 per row
  alternate  every second weight zero
  tiny       the 'random' knots as t * 1e-3 + 0.5: tiny intervals far from the origin, where midpoint differences cancel
"""
import numpy as np

KINDS = ("random", "plateau", "zero", "onehot", "alternate", "tiny")
EPS32 = float(np.finfo(np.float32).eps)
LANES = 64


def rows(kind, R, N, seed):
    g = np.random.default_rng([11, KINDS.index(kind), R, N, seed])
    t = np.sort(g.random((R, N + 1)), -1)
    t[:, 0], t[:, -1] = 0.0, 1.0
    t = t.astype(np.float32)
    e = np.exp(2.0 * g.standard_normal((R, N)))
    w = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    if kind == "plateau":
        for r in range(R):
            k = int(g.integers(0, max(N - 1, 1)))
            t[r, k + 1:min(k + 3, N + 1)] = t[r, k]
        assert (np.diff(t, axis=-1) >= 0).all()
    elif kind == "zero":
        w[:] = 0.0
    elif kind == "onehot":
        w[:] = 0.0
        w[np.arange(R), g.integers(0, N, R)] = 1.0
    elif kind == "alternate":
        w[:, (seed % 2)::2] = 0.0
    elif kind == "tiny":
        t = (t * np.float32(1e-3) + np.float32(0.5)).astype(np.float32)
        assert (np.diff(t, axis=-1) >= 0).all()
    return np.ascontiguousarray(t), np.ascontiguousarray(w)


def run_length(N):
    """intervals per lane of the kernels' layout: lane l owns [l C, min((l + 1) C, N)), C = ceil(N / 64)"""
    return (N + LANES - 1) // LANES


def two_hot_pairs(N):
    """(i, j), i < j: the ends, the first two, the last two, every pair of neighbours that straddles two lanes' runs, and the
    first and the last interval against the first interval of every lane at a power-of-two distance (the strides of the
    64-lane scans, from below and from above)."""
    if N < 2:
        return []
    C = run_length(N)
    pairs = {(0, N - 1), (0, 1), (N - 2, N - 1)}
    for lane in range(1, LANES):
        b = lane * C
        if b < N:
            pairs.add((b - 1, b))
            if lane & (lane - 1) == 0:
                pairs.add((0, b))
                if b < N - 1:
                    pairs.add((b, N - 1))
    return sorted(pairs)


def two_hot_rows(N, seed=0):
    """one row per pair of two_hot_pairs(N): weight 0.5 on the two intervals, 'random' knots"""
    pairs = two_hot_pairs(N)
    t, _ = rows("random", len(pairs), N, 1000 + seed)
    w = np.zeros((len(pairs), N), np.float32)
    for r, (i, j) in enumerate(pairs):
        w[r, i] = w[r, j] = 0.5
    return t, w, pairs


def truth(t, w):
    """The O(N^2) definition in float64 on the float32 inputs: (per-ray loss [R], d loss / d w [R, N]).
    loss = sum_ij w_i w_j |u_i - u_j| + (1/3) sum_i w_i^2 (t_{i+1} - t_i); its w-gradient is
    2 sum_j w_j |u_k - u_j| + (2/3) w_k (t_{k+1} - t_k)."""
    t, w = np.asarray(t, np.float64), np.asarray(w, np.float64)
    loss, grad = np.empty(t.shape[0]), np.empty(w.shape)
    for a in range(0, t.shape[0], 8):           # [8, N, N] at a time
        tb, wb = t[a:a + 8], w[a:a + 8]
        u = (tb[:, 1:] + tb[:, :-1]) / 2
        d = tb[:, 1:] - tb[:, :-1]
        inner = (np.abs(u[:, :, None] - u[:, None, :]) * wb[:, None, :]).sum(-1)
        loss[a:a + 8] = (wb * inner).sum(-1) + (wb * wb * d).sum(-1) / 3
        grad[a:a + 8] = 2 * inner + 2 * wb * d / 3
    return loss, grad


def bound(N):
    """(2N + 16) eps32, relative: loss and gradient are sums of at most 2N non-negative products of fp32 inputs, so this
    holds for any summation order"""
    return (2 * N + 16) * EPS32
