"""Float64 / exact numpy restatements of the stage-5 definitions (csrc/evaluate.hip, jatts_amd/evaluate.py): what the
evaluation kernels are pinned on.  numpy only; nothing here comes from the reference, whose stage 5 needs libraries that are absent
(parity with WORLD, Harvest, fastdtw and librosa.effects.trim is UNPINNED)."""
import itertools
import math

import numpy as np

MCD_SCALE = 10.0 / math.log(10.0)


# ---- step 2: cepstra
def dct_matrix(n_in=80, n_out=40):
    """float64 (n_out, n_in): the orthonormal DCT-II, row c = s_c cos(pi (k + 1/2) c / n_in), s_0 = sqrt(1 / n_in), else sqrt(2 / n_in)."""
    k = np.arange(n_in, dtype=np.float64)[None, :]
    c = np.arange(n_out, dtype=np.float64)[:, None]
    w = np.cos(np.pi * (k + 0.5) * c / n_in) * math.sqrt(2.0 / n_in)
    w[0] *= math.sqrt(0.5)
    return w


def cepstra(logmel, n_out=40):
    """float64 (T, n_out) of a (T, n_mels) log-mel"""
    m = np.asarray(logmel, dtype=np.float64)
    return m @ dct_matrix(m.shape[1], n_out).T


# ---- steps 3, 4, 9: frame selection
def select_mean(val, factor):
    """indices with val > factor * mean (float64)"""
    v = np.asarray(val, dtype=np.float64)
    return np.nonzero(v > factor * v.mean())[0].astype(np.int32)


def select_positive(val):
    return np.nonzero(np.asarray(val, dtype=np.float64) > 0.0)[0].astype(np.int32)


def select_max(val, factor):
    """(first, last) index with val > factor * max, (-1, -1) when none"""
    v = np.asarray(val, dtype=np.float64)
    sel = np.nonzero(v > factor * v.max())[0]
    return (int(sel[0]), int(sel[-1])) if sel.size else (-1, -1)


def threshold_margin(val, threshold):
    """min over frames of |val - threshold| / |threshold| (inf for a zero threshold): the tests require > 1e-9 of their inputs"""
    v = np.asarray(val, dtype=np.float64)
    return float(np.min(np.abs(v - threshold)) / abs(threshold)) if threshold != 0.0 else math.inf


def trimmed_length(pow_sum, n_samples, hop=512, top_db=60.0):
    """step 9 from the frame powers of an Stft(2048, hop): min(n, (last + 1) hop) - first hop; 0 when nothing is selected"""
    first, last = select_max(pow_sum, 10.0 ** (-top_db / 10.0))
    return 0 if first < 0 else min(int(n_samples), (last + 1) * hop) - first * hop


# ---- step 5: exact DTW
def pairwise_dist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def dtw(cost):
    """The plain double loop: -> (path_i, path_j int32, D[N-1][M-1]).  float64 accumulation of the given costs; ties go to the diagonal,
    then (i - 1, j), then (i, j - 1)."""
    c = np.asarray(cost)
    n, m = c.shape
    D = np.full((n, m), np.inf)
    dec = np.zeros((n, m), dtype=np.int8)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                D[0, 0] = float(c[0, 0])
                continue
            best, k = (D[i - 1, j - 1], 0) if i > 0 and j > 0 else (np.inf, 0)
            if i > 0 and D[i - 1, j] < best:
                best, k = D[i - 1, j], 1
            if j > 0 and D[i, j - 1] < best:
                best, k = D[i, j - 1], 2
            D[i, j] = float(c[i, j]) + best
            dec[i, j] = k
    return (*backtrack(dec), float(D[-1, -1]))


def backtrack(dec):
    i, j = dec.shape[0] - 1, dec.shape[1] - 1
    pi, pj = [i], [j]
    while i or j:
        k = dec[i, j]
        if k == 0:
            i, j = i - 1, j - 1
        elif k == 1:
            i -= 1
        else:
            j -= 1
        pi.append(i)
        pj.append(j)
    return np.array(pi[::-1], dtype=np.int32), np.array(pj[::-1], dtype=np.int32)


def dtw_fast(cost):
    """dtw() one anti-diagonal at a time: the same float64 adds of the same values (a minimum is exact), so the same bits; for the sizes
    the double loop is too slow for.  tests/test_evaluate_cpu.py holds the two equal."""
    c = np.asarray(cost)
    n, m = c.shape
    cd = c.astype(np.float64)
    D = np.full((n + 1, m + 1), np.inf)       # D[i + 1][j + 1] = the cell (i, j)
    dec = np.zeros((n, m), dtype=np.int8)
    for d in range(n + m - 1):
        i = np.arange(max(0, d - m + 1), min(n - 1, d) + 1)
        j = d - i
        dg, up, lf = D[i, j], D[i, j + 1], D[i + 1, j]
        best, k = dg.copy(), np.zeros(i.size, dtype=np.int8)
        t = up < best
        best[t], k[t] = up[t], 1
        t = lf < best
        best[t], k[t] = lf[t], 2
        if d == 0:
            best[:] = 0.0
        D[i + 1, j + 1] = cd[i, j] + best
        dec[i, j] = k
    return (*backtrack(dec), float(D[n, m]))


def monotone_paths(n, m):
    """Every warping path from (0, 0) to (n - 1, m - 1) with steps (1, 1), (1, 0), (0, 1), as lists of cells"""
    def rec(i, j):
        if i == n - 1 and j == m - 1:
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n and j + dj < m:
                for rest in rec(i + di, j + dj):
                    yield [(i, j)] + rest
    return list(rec(0, 0))


def tie_rule_path(cost):
    """Among ALL monotone paths: the one the tie rule picks, found without the recurrence's decisions -- walking back from the end, step to
    the first of (i-1, j-1), (i-1, j), (i, j-1) from which a minimal-cost prefix reaches the current cell.  Exact for integer costs."""
    c = np.asarray(cost, dtype=np.float64)
    n, m = c.shape
    best = {}                      # cell -> minimal cost of a path from (0, 0) to it, by enumeration of the prefixes
    for i, j in itertools.product(range(n), range(m)):
        best[i, j] = min(sum(c[a, b] for a, b in p) for p in monotone_paths(i + 1, j + 1))
    i, j = n - 1, m - 1
    path = [(i, j)]
    while i or j:
        cands = [(a, b) for a, b in ((i - 1, j - 1), (i - 1, j), (i, j - 1)) if a >= 0 and b >= 0]
        lo = min(best[q] for q in cands)
        i, j = next(q for q in cands if best[q] == lo)
        path.append((i, j))
    return path[::-1], best[n - 1, m - 1]


# ---- steps 6, 8: sums along the path
def path_terms(pi, pj, a=None, b=None, x=None, y=None):
    """-> dict of the per-step float64 terms the kernel sums: "mcd" = sqrt(2 sum_c (a - b)^2) with c ascending, one rounding per product
    and per add; "x", "y", "xx", "yy", "xy", "dd"."""
    out = {}
    if a is not None:
        df = np.asarray(a, dtype=np.float64)[pi] - np.asarray(b, dtype=np.float64)[pj]
        s = np.zeros(df.shape[0])
        for c in range(df.shape[1]):
            s = s + df[:, c] * df[:, c]
        out["mcd"] = np.sqrt(2.0 * s)
    if x is not None:
        xv, yv = np.asarray(x, dtype=np.float64)[pi], np.asarray(y, dtype=np.float64)[pj]
        out.update(x=xv, y=yv, xx=xv * xv, yy=yv * yv, xy=xv * yv, dd=(xv - yv) * (xv - yv))
    return out


STAT_ORDER = ("mcd", "x", "y", "xx", "yy", "xy", "dd")       # columns 1 .. 7 of jatts_dtw_path_stats (column 0: L)


def metrics_from_sums(mcd_sums, f0_sums):
    """The host's last step (jatts_amd.evaluate.metrics_from_sums restated): -> (MCD, F0RMSE, F0CORR)"""
    mcd = MCD_SCALE * mcd_sums[1] / mcd_sums[0]
    if f0_sums is None:
        return mcd, math.nan, math.nan
    n, _, sx, sy, sxx, syy, sxy, sdd = f0_sums
    cov, vx, vy = sxy - sx * sy / n, sxx - sx * sx / n, syy - sy * sy / n
    corr = cov / math.sqrt(vx * vy) if vx > 0.0 and vy > 0.0 else math.nan
    return mcd, math.sqrt(sdd / n), corr


def evaluate_chain(cep_x, cep_y, pow_x, pow_y, f0_x, f0_y):
    """Steps 4-8 in float64 on given per-frame features (the cepstra already float64 DCTs of the log-mel) -> (MCD, F0RMSE, F0CORR, the
    power path)"""
    ax, ay = select_mean(pow_x, 1e-2), select_mean(pow_y, 1e-2)
    a, b = cep_x[ax], cep_y[ay]
    pi, pj, _ = dtw_fast(pairwise_dist(a, b))
    t = path_terms(pi, pj, a, b)
    mcd_sums = [float(pi.size), float(t["mcd"].sum())]
    vx, vy = select_positive(f0_x), select_positive(f0_y)
    f0_sums = None
    if vx.size and vy.size:
        qi, qj, _ = dtw_fast(pairwise_dist(cep_x[vx], cep_y[vy]))
        t = path_terms(qi, qj, x=np.asarray(f0_x)[vx], y=np.asarray(f0_y)[vy])
        f0_sums = [float(qi.size), 0.0] + [float(t[k].sum()) for k in STAT_ORDER[1:]]
    return (*metrics_from_sums(mcd_sums, f0_sums), (pi, pj))
