"""Float64 numpy restatement of the `motion` retrieval method (exemplars by a motion example; this project's own scoring: the
reference has no counterpart): the sweep's arithmetic, the query validation and the placement rule.  Nothing here imports the
product.

Sweep, for a query (qlat [4, n_q, D], weights w, speaker, bonus) and an entry (lat [4, L, D]) over the offsets o = 0 .. L - n_q:
    S_p(o) = sum_{c < n_q} sum_{k < D} (lat[p, o + c, k] - qlat[p, c, k])^2         here in float64 (the device: fp32)
    d(o)   = sum over the parts with w_p > 0, in order, of w_p * S_p(o)
    o*     = the offset of the smallest d, the lowest among equals
    score  = 1 / (1 + d(o*) / (n_q D (((w_0 + w_1) + w_2) + w_3))) + (spk == speaker ? bonus : 0);   top = o*
"""
import numpy as np

PARTS = 4
CHUNK, FPS, N_LAT = 15, 15, 10
DEFAULT_WEIGHTS = (1.0, 1.0, 0.0, 0.0)
EXAMPLE_KEYS = ("motion_upper", "motion_lower", "motion_face", "motion_hands", "trans", "facial", "contact")
RANK_MAX = 10


def part_sums(lat, qlat):
    """lat [n, 4, L, D], qlat [4, n_q, D] (any float type; differences taken in float64) -> S float64 [n, 4, L - n_q + 1]."""
    lat, qlat = np.asarray(lat, dtype=np.float64), np.asarray(qlat, dtype=np.float64)
    n, _, L, _ = lat.shape
    n_q = qlat.shape[1]
    S = np.empty((n, PARTS, L - n_q + 1), dtype=np.float64)
    for o in range(L - n_q + 1):
        diff = lat[:, :, o:o + n_q, :] - qlat[None]
        S[:, :, o] = (diff * diff).sum(axis=(2, 3))
    return S


def weight_sum(w):
    return ((np.float64(0.0) + np.float64(w[0]) + np.float64(w[1])) + np.float64(w[2])) + np.float64(w[3])


def distances(S, w):
    """S [n, 4, n_o] (float64 values; the device's fp32 sums converted) -> d float64 [n, n_o]: the weighted parts, in order."""
    d = np.zeros((S.shape[0], S.shape[2]), dtype=np.float64)
    for p in range(PARTS):
        if w[p] > 0:
            d = d + np.float64(w[p]) * S[:, p, :].astype(np.float64)
    return d


def score_of(d_best, n_q, D, w, spk, speaker, bonus):
    """d(o*) float64 [n] -> score float64 [n], operation for operation as the kernel states it."""
    dn = d_best / (np.float64(n_q * D) * weight_sum(w))
    sc = np.float64(1.0) / (np.float64(1.0) + dn)
    return np.where(np.asarray(spk) == int(speaker), sc + np.float64(bonus), sc)


def scores(lat, spk, qlat, w=DEFAULT_WEIGHTS, speaker=-1, bonus=0.0):
    """-> (score float64 [n], top int32 [n], S float64 [n, 4, n_o], d float64 [n, n_o]).  Parts without weight do not enter:
    their S is still returned (NaN where the table holds NaN) but never read."""
    qlat = np.asarray(qlat)
    S = part_sums(lat, qlat)
    d = distances(S, w)
    top = np.argmin(d, axis=1).astype(np.int32)            # the first minimum: the lowest offset among equals
    best = d[np.arange(d.shape[0]), top]
    return score_of(best, qlat.shape[1], qlat.shape[2], w, spk, speaker, bonus), top, S, d


def validate_query(query, chunk=CHUNK, n_lat=N_LAT):
    """(start_s, end_s, example[, weights]) -> (start_s, end_s, weights, n_q), or ValueError with the refusal's reason."""
    if len(query) not in (3, 4):
        raise ValueError("shape")
    start_s, end_s, example = float(query[0]), float(query[1]), query[2]
    if not start_s <= end_s:
        raise ValueError("start_s must be <= end_s")
    if any(k not in example for k in EXAMPLE_KEYS):
        raise ValueError("lacks")
    frames = {int(example[k].shape[0]) for k in EXAMPLE_KEYS}
    if len(frames) != 1:
        raise ValueError("different numbers of frames")
    frames = frames.pop()
    if frames % chunk:
        raise ValueError("not a multiple of the chunk")
    n_q = frames // chunk
    if not 1 <= n_q <= n_lat:
        raise ValueError("chunks out of range")
    w = DEFAULT_WEIGHTS if len(query) == 3 or query[3] is None else tuple(float(v) for v in query[3])
    if len(w) != PARTS or not all(np.isfinite(v) and v >= 0 for v in w):
        raise ValueError("weights must be finite and non-negative")
    if not any(v > 0 for v in w):
        raise ValueError("weights must not all be zero")
    return start_s, end_s, w, n_q


def place(queries, n_lat=N_LAT, chunk=CHUNK, fps=FPS):
    """The placement rule of the motion method for ONE clip with one exemplar per query: queries = [(start_s, end_s, o*, n_q)]
    in ascending start_s -> per query None (no room left) or ((r_lat_start, r_lat_end), (start_lat, end_lat)).
    The exemplar's chunk range is taken as it stands; the query side is centred on the query span's middle chunk by the
    reference's rule (one chunk: on it; two: from it; odd n: side + 1 chunks in front; even: side in front), clamped into the
    window, and pushed behind the previous exemplar (shortened at the window's end, dropped if nothing is left)."""
    out, prev_end = [], -1
    motion_len = n_lat * chunk
    for start_s, end_s, o, n_q in queries:
        qs, qe = int(max(0, start_s) * fps), int(min(motion_len / fps, end_s) * fps)
        r0, r1 = o, o + n_q
        mid = ((qs + qe) // 2) // chunk
        n, side = n_q, n_q // 2
        if n == 1:
            s, e = mid, mid + 1
        elif n == 2:
            s, e = mid, mid + 2
        elif n % 2 == 1:
            s, e = mid - side - 1, mid + side
        else:
            s, e = mid - side, mid + side
        if s < 0:
            s, e = 0, n
        if e > n_lat:
            s, e = s - (e - n_lat), n_lat
        if s < prev_end:
            s = prev_end
            e = s + n
            if e > n_lat:
                e = n_lat
                n = e - s
                if n <= 0:
                    out.append(None)
                    continue
                r1 = r0 + n
        prev_end = e
        out.append(((r0, r1), (s, e)))
    return out


def ranking_walk(score, tie_sim):
    """score float64 [n]; tie_sim(entry) -> similarity.  Entries of positive score by descending score (entry order inside a
    tier); the leading tiers while fewer than RANK_MAX are held; a multi-member tier reordered by descending similarity, stable."""
    order = sorted((e for e in range(len(score)) if score[e] > 0), key=lambda e: -score[e])
    ranked, i = [], 0
    while i < len(order) and len(ranked) < RANK_MAX:
        j = i
        while j < len(order) and score[order[j]] == score[order[i]]:
            j += 1
        tier = order[i:j]
        if len(tier) > 1:
            sims = {e: tie_sim(e) for e in tier}
            tier = sorted(tier, key=lambda e: -sims[e])
        ranked += tier
        i = j
    return ranked[:RANK_MAX]


def text_similarity(q, f):
    """mean_i q[i] . f[i] over the common rows: fp32 products summed in float64."""
    n = min(q.shape[0], f.shape[0])
    if n == 0:
        return 0.0
    return float((np.asarray(q[:n], dtype=np.float32) * np.asarray(f[:n], dtype=np.float32)).astype(np.float64).sum() / n)


def fixture(seed, n, L=N_LAT, D=512, n_qs=(1, 2, 3, 7, 10)):
    """The kernel tests' data: a standard-normal table [n, 4, L, D] and queries [4, n_q, D], every chunk (row of D values)
    scaled by a factor drawn from [0.25, 4] (log-uniform) so that neighbouring offsets' distances are rarely close; speakers 0..2."""
    g = np.random.Generator(np.random.PCG64(seed))
    scale = lambda shape: np.exp(g.uniform(np.log(0.25), np.log(4.0), size=shape)).astype(np.float32)
    lat = g.standard_normal((n, PARTS, L, D)).astype(np.float32) * scale((n, PARTS, L, 1))
    qlats = [g.standard_normal((PARTS, k, D)).astype(np.float32) * scale((PARTS, k, 1)) for k in n_qs]
    spk = g.integers(0, 3, size=n).astype(np.int32)
    return lat, spk, qlats


def sum_bound(n_q, D):
    """Relative error bound of the device's fp32 S_p: a sum of n_q D non-negative terms, each one subtraction (one rounding) and
    one fused multiply-add (one rounding per addition into the sum): (n_q D + 2) 2^-24, whatever the order of the additions."""
    return (n_q * D + 2) * 2.0 ** -24
