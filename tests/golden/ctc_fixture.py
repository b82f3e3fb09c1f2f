"""Float64 NumPy restatement of what rag-gesture_amd/align.py and csrc/rg_ctc.hip compute (tests/test_align_cpu.py,
tests/test_align_gpu.py): the log-softmax, the CTC Viterbi recurrence with its tie rule and back-track, the token and time
rules, greedy decoding, and the reference's frame alignment of word vectors (mogen/datasets/beatx_dataset.py:865-869 with
get_word_vectors' mean, :1155-1156).  Nothing here imports the package."""
import numpy as np

SAMPLE_RATE, FRAME_STRIDE, FRAME_FIELD = 16000, 320, 400
VOCAB = {"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "|": 4, "E": 5, "T": 6, "A": 7, "O": 8, "N": 9, "I": 10, "H": 11, "S": 12,
         "R": 13, "D": 14, "L": 15, "U": 16, "M": 17, "W": 18, "C": 19, "F": 20, "G": 21, "Y": 22, "P": 23, "B": 24, "V": 25,
         "K": 26, "'": 27, "X": 28, "J": 29, "Q": 30, "Z": 31}            # the layout of a character CTC vocabulary
BLANK, DELIMITER = 0, "|"


def log_softmax(x):
    x = np.asarray(x, np.float64)
    d = x - x.max(-1, keepdims=True)
    return d - np.log(np.exp(d).sum(-1, keepdims=True))


def viterbi(E, y, blank=BLANK, dtype=np.float64):
    """E [T, V] emissions, y [L] tokens -> dict(path [T], tok_first [L], tok_last [L], score, status), all arithmetic in dtype.
    The recurrence of include/rg_gesture.h (rg_ctc_align): candidates stay (code 0), one back (1), two back (2, only into a
    token state whose token differs from the one two back), a strictly greater value replaces."""
    E = np.asarray(E, dtype)
    T, L = E.shape[0], len(y)
    S = 2 * L + 1
    z = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    NEG = dtype(-np.inf)
    a = np.full(S, NEG, dtype)
    a[0] = E[0, blank]
    a[1] = E[0, z[1]]
    back = np.zeros((T, S), np.int8)
    zi = np.asarray(z)
    skip_ok = np.array([s >= 2 and z[s] != blank and z[s] != z[s - 2] for s in range(S)])
    for t in range(1, T):                                     # (all states of a frame at once: the same comparisons per state)
        one = np.concatenate([[NEG], a[:-1]])                 # a[t - 1][s - 1], absent for s = 0
        two = np.concatenate([[NEG, NEG], a[:-2]])
        best, code = a.copy(), np.zeros(S, np.int8)
        m = one > best
        best[m], code[m] = one[m], 1
        m = skip_ok & (two > best)
        best[m], code[m] = two[m], 2
        a = (E[t, zi] + best).astype(dtype)
        back[t] = code
    s = S - 1
    if S > 1 and a[S - 2] > a[S - 1]:
        s = S - 2
    score = a[s]
    if not score > NEG:
        return dict(path=np.zeros(T, np.int32), tok_first=np.full(L, -1, np.int32), tok_last=np.full(L, -1, np.int32),
                    score=np.float32(score), status=1)
    path = np.zeros(T, np.int32)
    for t in range(T - 1, -1, -1):
        path[t] = s
        if t:
            s -= int(back[t, s])
    first, last = np.full(L, -1, np.int32), np.full(L, -1, np.int32)
    for t, st in enumerate(path):
        if st % 2:
            if first[st // 2] < 0:
                first[st // 2] = t
            last[st // 2] = t
    return dict(path=path, tok_first=first, tok_last=last, score=np.float32(score), status=0)


def path_is_valid(path, y, blank=BLANK):
    """Starts in state 0 or 1, ends in S - 1 or S - 2, steps by 0, 1 or 2, a 2-step only into a token state whose token differs
    from the one two back; visits every token state."""
    S = 2 * len(y) + 1
    z = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    p = [int(s) for s in path]
    if p[0] not in (0, 1) or p[-1] not in (S - 1, S - 2):
        return False
    for u, v in zip(p[:-1], p[1:]):
        if v - u not in (0, 1, 2) or (v - u == 2 and (z[v] == blank or z[v] == z[u])):
            return False
    return set(range(1, S, 2)) <= set(p)


def path_score(E, path, y, blank=BLANK):
    """The sum of a path's emissions in float64."""
    S = 2 * len(y) + 1
    z = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    return float(sum(np.float64(E[t, z[int(s)]]) for t, s in enumerate(path)))


def exact_emissions(rng, T, V):
    """Multiples of 1/8 in [-16, 0]: every fp32 sum of up to 2^13 of them is exact, so fp32 and fp64 agree bit for bit."""
    return (-rng.integers(0, 129, size=(T, V)) / 8.0).astype(np.float32)


def random_tokens(rng, L, V, blank=BLANK, kind="mixed"):
    """kind: "mixed" (about a third of the positions repeat their neighbour), "equal" (one class), "distinct" (no repeats)."""
    classes = [c for c in range(V) if c != blank]
    if kind == "equal":
        return [classes[0]] * L
    y = []
    for j in range(L):
        if j and kind == "mixed" and rng.random() < 0.33:
            y.append(y[-1])
        else:
            y.append(int(rng.choice([c for c in classes if not y or c != y[-1]])))
    return y


def planted_path(rng, T, y, blank=BLANK):
    """A random valid state path of T frames for tokens y (T large enough), and the emissions that make it the unique optimum:
    E[t][z[path[t]]] = 0, every other class -4 (V = the VOCAB's)."""
    L = len(y)
    S = 2 * L + 1
    z = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    # the states the path visits: every token state; a blank state where it must (between equal tokens) or by a coin
    visited = [s for s in range(S) if s % 2 or (0 < s < S - 1 and y[s // 2 - 1] == y[s // 2]) or rng.random() < 0.5]
    while len(visited) > T:                                   # (too many optional blanks for T frames: drop some)
        optional = [s for s in visited if s % 2 == 0 and not (0 < s < S - 1 and y[s // 2 - 1] == y[s // 2])]
        visited.remove(optional[int(rng.integers(len(optional)))])
    cuts = np.sort(rng.choice(np.arange(1, T), size=len(visited) - 1, replace=False)) if len(visited) > 1 else np.zeros(0, int)
    runs = np.diff(np.concatenate([[0], cuts, [T]])).astype(int)
    path = [s for s, n in zip(visited, runs) for _ in range(n)]
    assert len(path) == T and path_is_valid(path, y, blank)
    E = np.full((T, len(VOCAB)), -4.0, np.float32)
    for t, s in enumerate(path):
        E[t, z[s]] = 0.0
    return np.asarray(path, np.int32), E


# ------------------------------------------------------------------------------------------------ text and time
def tokens(words, vocab=VOCAB, blank=BLANK, delimiter=DELIMITER):
    chars = {c: i for c, i in vocab.items() if len(c) == 1 and i != blank and c != delimiter}
    ids, word_of = [], []
    for w, word in enumerate(words):
        got = []
        for ch in word:
            ch = "'" if ch == "’" else ch
            for c in (ch, ch.upper(), ch.lower()):
                if len(c) == 1 and c in chars:
                    got.append(chars[c])
                    break
        if not got:
            continue
        if ids:
            ids.append(vocab[delimiter])
            word_of.append(-1)
        ids += got
        word_of += [w] * len(got)
    return ids, word_of


def word_times(words, word_of, first, last, frame_sample, n_samples):
    total = n_samples / SAMPLE_RATE
    spans = {}
    for k, w in enumerate(word_of):
        if w < 0:
            continue
        s, e = frame_sample[first[k]] / SAMPLE_RATE, min((frame_sample[last[k]] + FRAME_STRIDE) / SAMPLE_RATE, total)
        spans[w] = [spans[w][0], e] if w in spans else [s, e]
    out = []
    for i, word in enumerate(words):
        if i in spans:
            out.append([spans[i], word])
            continue
        before = [spans[j][1] for j in range(i) if j in spans]
        after = [spans[j][0] for j in range(i + 1, len(words)) if j in spans]
        out.append([[before[-1] if before else 0.0, after[0] if after else total], word])
    return out


def greedy(best, blank=BLANK, delimiter_id=VOCAB[DELIMITER]):
    """-> words as lists of (class, first frame, last frame)."""
    runs, t = [], 0
    best = [int(b) for b in best]
    while t < len(best):
        u = t
        while u + 1 < len(best) and best[u + 1] == best[t]:
            u += 1
        runs.append((best[t], t, u))
        t = u + 1
    words, cur = [], []
    for c, a, b in runs:
        if c == blank:
            continue
        if c == delimiter_id:
            if cur:
                words.append(cur)
            cur = []
        else:
            cur.append((c, a, b))
    if cur:
        words.append(cur)
    return words


# ------------------------------------------------------------------------------------------------ frame alignment
def word_frames(hidden, groups, segments, n_frames, pose_fps=15):
    """hidden [L, D] token rows; groups[w] = the token positions of word w; segments[w] = [[start, end], word].
    mogen/datasets/beatx_dataset.py:865-869: zeros, then in word order smp[int(start fps):int(end fps)] = mean of the rows."""
    hidden = np.asarray(hidden, np.float64)
    smp = np.zeros((n_frames, hidden.shape[1]))
    for w, seg in enumerate(segments):
        vec = hidden[groups[w]].mean(0)
        start_frame, end_frame = int(seg[0][0] * pose_fps), int(seg[0][1] * pose_fps)
        smp[start_frame:end_frame] = vec
    return smp


def word_frames_bound(hidden, groups, segments, n_frames, pose_fps=15):
    """Per component 2^-23 sum_j |x_j| over the rows of the word that owns the frame (n - 1 roundings of partial sums that never
    exceed sum |x_j|, one of the division, each at most 2^-24 relative: n 2^-24 sum |x_j| / n <= this); 0 where no word does."""
    hidden = np.abs(np.asarray(hidden, np.float64))
    b = np.zeros((n_frames, hidden.shape[1]))
    for w, seg in enumerate(segments):
        b[int(seg[0][0] * pose_fps):int(seg[0][1] * pose_fps)] = 2.0 ** -23 * hidden[groups[w]].sum(0)
    return b
