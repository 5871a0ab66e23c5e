"""The co-fragmentation rule of ``include/ftk.h`` ("co-fragmentation") restated for the tests: ``ks_matrix`` in
vectorised numpy and, behind it, ``ks_matrix_loop``, a per-pair loop in Python integers that cannot overflow - the CPU
tests hold the two to each other, also where the products reach (2^31 - 1)^2 and numpy's int64 would not be trusted
alone.  Plus the planted-compartment histograms of the issue.  Nothing here calls the library."""
import numpy as np

MAX_BINS = 4096
ROW_LIMIT = 1 << 31


def ks_matrix_loop(hist):
    """``(K, at, n)`` by the letter of the rule, in Python integers: lists of lists and a list."""
    rows = [[int(v) for v in r] for r in np.asarray(hist)]
    n = [sum(r) for r in rows]
    pre = []
    for r in rows:
        c, acc = [], 0
        for v in r:
            acc += v
            c.append(acc)
        pre.append(c)
    N = len(rows)
    K = [[0] * N for _ in range(N)]
    at = [[0] * N for _ in range(N)]
    for i in range(N):
        for j in range(N):
            best, where = 0, 0
            for l, (ci, cj) in enumerate(zip(pre[i], pre[j])):
                v = abs(ci * n[j] - cj * n[i])
                if v > best:
                    best, where = v, l
            K[i][j], at[i][j] = best, where
    return K, at, n


def ks_matrix(hist):
    """``(K int64 [N, N], at int32 [N, N], n int64 [N])`` of uint32 rows whose sums are below 2^31: every product is below
    2^62 and the difference of two fits int64, so the arithmetic is exact.  ``argmax`` returns the first maximum."""
    h = np.asarray(hist, dtype=np.uint32)
    N = h.shape[0]
    C = np.cumsum(h.astype(np.int64), axis=1)
    n = C[:, -1].copy()
    assert (n < ROW_LIMIT).all()
    K = np.zeros((N, N), np.int64)
    at = np.zeros((N, N), np.int32)
    for i in range(N):
        v = np.abs(C[i][None, :] * n[:, None] - C * n[i])  # [j, l]
        at[i] = np.argmax(v, axis=1)
        K[i] = v[np.arange(N), at[i]]
    return K, at, n


def random_hist(rng, n_rows, n_bins, top=40):
    return rng.integers(0, top, (n_rows, n_bins)).astype(np.uint32)


# ---- planted compartments: 24 bins in the pattern 5 A, 4 B, 6 A, 9 B over 64 lengths
PLANTED_GROUPS = np.array([0] * 5 + [1] * 4 + [0] * 6 + [1] * 9)


def planted_hist(depth, seed=7):
    """Row i: a multinomial draw of ``depth + 37 i`` fragments from a discretised Gaussian, sigma 6, at length 28 (group
    A) or 36 (group B)."""
    rng = np.random.default_rng(seed)
    l = np.arange(64)
    rows = []
    for i, g in enumerate(PLANTED_GROUPS):
        p = np.exp(-0.5 * ((l - (28 if g == 0 else 36)) / 6.0) ** 2)
        rows.append(rng.multinomial(depth + 37 * i, p / p.sum()))
    return np.array(rows, np.uint32)
