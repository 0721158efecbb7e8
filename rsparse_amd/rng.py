"""The counter-based normal generator behind `WRMF(factor_init="device")`, in numpy: the specification of the stream that
rsparse_amd/csrc/wrmf_init.hip draws on the device (include/rsparse_wrmf_hip.h states the same definition for C hosts), the
oracle of its tests, and the fallback of a backend that has no device.

    bits      Philox4x32-10 (Random123): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85
    index     the matrix is (n_rows, rank) row-major; e = row * rank + col, 64 bits, over the WHOLE matrix
    counter   (lo32(e >> 2), hi32(e >> 2), stream, 0);   key (lo32(seed), hi32(seed));   stream 0 = users, 1 = items
    outputs   one call gives o0..o3 and four normals; element e takes number e & 3
    uniforms  u_a = ((o0 >> 8) + 1) 2^-24 in (0, 1],  u_b = (o1 >> 8) 2^-24 in [0, 1)        (exact in fp32)
    normals   r = sqrt(-2 ln u_a);  numbers 0, 1 = r cos(2 pi u_b), r sin(2 pi u_b);  2, 3 the same from (o2, o3)
    value     scale * z, |.| with abs_values; the column ones_col (-1: none) is exactly 1

A value depends on (seed, stream, row, col, rank) alone: not on the row range asked for, the number of ranks or the device.
Evaluated in float64 and cast at the end.  |z| <= sqrt(48 ln 2) = 5.77; z is exactly 0 only for u_a = 1 (one pair in 2^24) or
at a quarter turn of u_b (four values in 2^24).

`sample_negatives` is the specification of the third stream of the same generator: per-row uniform samples WITHOUT replacement of
the items outside a row's exclusion list (rsparse_amd/csrc/wrmf_sample.hip draws it on the device, bit for bit; the header states
it for C hosts).  For the row with global index g, seen = its sorted unique exclusion list, keep = the sorted unique items copied
into the output (a subset of seen), M = n_item - |seen| admissible items numbered by RANK 0 .. M - 1 in ascending item order:

    item(r)   r + #{i : seen[i] - i <= r}                     (a binary search: seen[i] - i does not decrease)
    draw t    Philox4x32-10, key (lo32(seed), hi32(seed)), counter (lo32(t >> 1), g, 2, hi32(t >> 1)) -> o0..o3;
              w = o1 2^32 + o0 for even t, o3 2^32 + o2 for odd t;  rank = floor(w M / 2^64) = (o_hi M + ((o_lo M) >> 32)) >> 32
              (exact in 64-bit unsigned arithmetic for M < 2^31; bias at most M / 2^64)
    chosen    n >= M: every rank.  Otherwise d = min(n, M - n) and D = the first d DISTINCT values of the draw sequence
              t = 0, 1, 2, ...; the chosen ranks are D when 2 n <= M and every rank but D otherwise (the row then draws what it
              leaves out: no row needs more than about M ln 2 draws)
    row       the ascending merge of keep and the items of the chosen ranks: |keep| + min(n, M) entries

The negatives depend on (seed, g, seen, n_item, n) alone: not on the rows asked for together, the device, or the order in which
the draws are evaluated ("the first d distinct values" is a property of the sequence).

`sample_negatives_weighted` is the specification of the sixth stream: the same rows with the negatives drawn in proportion to
integer item weights (popularity-weighted negatives; rsparse_amd/csrc/wrmf_sample_weighted.hip draws it on the device bit for
bit, the header states it for C hosts).  w[0 .. n_item) are unsigned 32-bit integers, every one >= 1 (a zero is refused: "never a
negative" is the job of the exclusion list); C[i] = w[0] + ... + w[i] in 64 bits, W = C[n_item - 1] < 2^63:

    draw t    Philox4x32-10, key (lo32(seed), hi32(seed)), counter (lo32(t >> 1), g, 5, hi32(t >> 1)) -> o0..o3;
              v = o1 2^32 + o0 for even t, o3 2^32 + o2 for odd t;  r = floor(v W / 2^64), the high 64 bits of the 128-bit
              product;  item = #{i : C[i] <= r} = searchsorted(C, r, side="right")
    chosen    M = n_item - |seen|.  n >= M: every admissible item, nothing is drawn.  Otherwise A = the first n DISTINCT values,
              in the order of the draw sequence, among the draws t = 0 .. B(n) - 1 that are NOT in seen, B(n) = 64 n + 4096.  If
              the budget ends with |A| < n the row is FILLED with the n - |A| admissible items of lowest item number that are
              not in A, and counts as a filled row (the budget is part of the definition: no input can make a row spin;
              ordinary weights never fill, weights such as [2^31, 1, 1, ...] do)
    row       the ascending merge of keep and the chosen items: |keep| + min(n, M) entries, as for the uniform sampler

A row depends on (seed, g, seen, keep, w, n) alone: not on the rows sampled with it, the batch, the rank count or the device.

`split_flags` / `split_rows` are the specification of the fourth and fifth stream: the train / test split of a canonical CSR
(columns ascending and unique per row; stored zeros count as entries), which rsparse_amd/csrc/wrmf_split.hip draws on the device
bit for bit.  Row u has the global index g = row0 + u and L entries; an entry is named by its position t = 0 .. L - 1 in the row:

    proportion   Philox4x32-10, key (lo32(seed), hi32(seed)), counter (t >> 2, g, 3, 0) -> o0..o3; the entry takes word o[t & 3]
                 and is TEST iff word < T (in 64 bits), T = floor(p 2^32) an integer in [0, 2^32]: T = 0 nothing, 2^32 everything
    leave-out    exactly h = min(n, max(L - min_train, 0)) entries of the row are test: every entry has a 64-bit key w, and the
                 test entries are the first h of the total order "a before b iff w_a > w_b, or w_a = w_b and t_a < t_b"
      random     counter (t >> 1, g, 4, 0); w = o1 2^32 + o0 for even t, o3 2^32 + o2 for odd t (the negatives' word pairing)
      by         one float64 per stored entry (a timestamp); u = its bits, w = ~u if the sign bit is set, else u | 2^63: the
                 order-preserving map, so the h LARGEST values are held out and ties go to the lower position; -0.0 orders
                 just below +0.0; NaN is refused; no random word is used

A flag depends on (seed, g, t, the mode's parameters) and, in leave-out mode, on the row's L or `by` values: not on the rows split
together, the batch, the rank count or the device.  row0 + n_rows <= 2^32, L < 2^31.

`STREAM_BPR` is the seventh stream: the (user, positive, negative) triples of the BPR fit (rsparse_amd/bpr.py: `bpr_triples` is the
numpy form, rsparse_amd/csrc/wrmf_bpr.hip draws them on the device bit for bit).  An epoch has one triple per stored entry of a
canonical CSR; slot p belongs to row u of L entries at position q = p - indptr[u]:

    counter   (q, g, 6, epoch + 2^31 mode), key (lo32(seed), hi32(seed)) -> o0..o3;  mode 0 = the fit, g = row0 + u;
              mode 1 = the fold-in, g = row0 for every row (a folded-in row's triples depend on the row alone; all rows of a
              fold-in epoch then share the words of a position q, hence its three negative candidates -- harmless with the items
              frozen, where no row sees another's update)
    positive  indices[indptr[u] + ((o0 L) >> 32)]
    negative  the first of (o1 n_items) >> 32, (o2 n_items) >> 32, (o3 n_items) >> 32 that is not in the row (a binary search);
              all three in the row: the triple is VOID (-1) and takes no part in anything -- no input can make the sampler spin

Integers only.  A triple depends on (seed, mode, epoch, g, q, the row, n_items) alone.  epoch < 2^31.
"""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
STREAM_USERS, STREAM_ITEMS, STREAM_NEGATIVES = 0, 1, 2
STREAM_SPLIT, STREAM_LEAVE_OUT = 3, 4
STREAM_WEIGHTED_NEGATIVES = 5
STREAM_BPR = 6
MAX_NEGATIVES = 8192   # RSPARSE_HIP_MAX_NEGATIVES
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds.  counter: (..., 4) and key: (..., 2) arrays of 32-bit words (broadcast against each other)
    -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j], shape) for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j], shape) for j in range(2))
    for rnd in range(10):
        if rnd:
            k0 = (k0 + np.uint64(PHILOX_W0)) & _MASK
            k1 = (k1 + np.uint64(PHILOX_W1)) & _MASK
        p0 = np.uint64(PHILOX_M0) * c0      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _cos_sin_2pi(m):
    """cos and sin of 2 pi m / 2^24 for integers 0 <= m < 2^24.  The quarter turn is taken off exactly, so the argument of the
    library call is at most pi / 4 and carries one rounding (absolute error below 2e-16, where cos(2 * pi * u) loses 1e-15),
    and the values at the quarter turns are exact, as a sincospi gives them."""
    m = m.astype(np.int64)
    q = (m + (1 << 21)) >> 22                      # nearest quarter turn (2^22 steps): 0..4
    a = (m - (q << 22)).astype(np.float64) * (np.pi / float(1 << 23))
    c, s = np.cos(a), np.sin(a)
    q = q & 3
    return np.choose(q, [c, -s, -c, s]), np.choose(q, [s, c, -s, -c])


def box_muller(words):
    """(..., 4) uint32 Philox outputs -> ((..., 4) float64 standard normals, (..., 4) their radii r)"""
    w = np.asarray(words, dtype=np.uint32)
    z = np.empty(w.shape, dtype=np.float64)
    rad = np.empty(w.shape, dtype=np.float64)
    for h in (0, 2):
        ua = ((w[..., h] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(ua))
        c, s = _cos_sin_2pi(w[..., h + 1] >> np.uint32(8))
        z[..., h], z[..., h + 1] = r * c, r * s
        rad[..., h] = rad[..., h + 1] = r
    return z, rad


def init_factors(seed, stream, row0, n_rows, rank, scale=0.01, abs_values=False, ones_col=-1, dtype=np.float64,
                 return_radius=False):
    """Rows [row0, row0 + n_rows) of the (anything, rank) matrix of stream `stream` under `seed`: an (n_rows, rank) array of
    `dtype`.  return_radius=True also gives the Box-Muller radius r of every element (float64; what an error bound of a lower
    precision evaluation scales with)."""
    seed, stream, row0, n_rows, rank, ones_col = int(seed), int(stream), int(row0), int(n_rows), int(rank), int(ones_col)
    if n_rows < 0 or row0 < 0 or rank < 1 or stream not in (0, 1) or not -1 <= ones_col < rank or not 0 <= seed < 2 ** 64:
        raise ValueError("init_factors: bad arguments")
    e0, e1 = row0 * rank, (row0 + n_rows) * rank
    g0, g1 = e0 >> 2, (e1 + 3) >> 2
    g = np.arange(g0, g1, dtype=np.uint64)
    counter = np.stack([g & _MASK, g >> _S32, np.full_like(g, stream), np.zeros_like(g)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    z, rad = box_muller(philox4x32_10(counter, key))
    lo, hi = e0 - 4 * g0, e1 - 4 * g0
    out = (float(scale) * z.reshape(-1)[lo:hi]).reshape(n_rows, rank)
    if abs_values:
        out = np.abs(out)
    if ones_col >= 0:
        out[:, ones_col] = 1.0
    out = out.astype(dtype)
    if return_radius:
        return out, rad.reshape(-1)[lo:hi].reshape(n_rows, rank)
    return out


def negative_draws(seed, g, t0, count, M):
    """the ranks of the draws t0 .. t0 + count - 1 of global row g among M admissible items -> uint64 array"""
    t = np.arange(t0, t0 + count, dtype=np.uint64)
    c = t >> np.uint64(1)
    counter = np.stack([c & _MASK, np.full_like(c, g), np.full_like(c, STREAM_NEGATIVES), c >> _S32], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    o = philox4x32_10(counter, key).astype(np.uint64)
    odd = (t & np.uint64(1)).astype(bool)
    lo, hi = np.where(odd, o[:, 2], o[:, 0]), np.where(odd, o[:, 3], o[:, 1])
    m = np.uint64(M)
    return (hi * m + ((lo * m) >> _S32)) >> _S32       # hi M < 2^63 and the carry < 2^31: no overflow


def first_distinct(seed, g, M, d):
    """the first d distinct ranks of row g's draw sequence, in the order of their first occurrence (needs d <= M)"""
    drawn = np.zeros(0, dtype=np.uint64)
    while True:
        step = max(64, 2 * d, drawn.size)
        drawn = np.concatenate([drawn, negative_draws(seed, g, drawn.size, step, M)])
        vals, first = np.unique(drawn, return_index=True)
        if vals.size >= d:
            return vals[np.argsort(first, kind="stable")[:d]].astype(np.int64)


def sample_negatives(seed, row0, seen_p, seen_j, keep_p, keep_j, n_item, n):
    """For every row u of the CSR pattern (seen_p, seen_j) -- global row row0 + u, columns sorted and unique --: the row's `keep`
    items (CSR (keep_p, keep_j), a subset of its seen items; both None = keep nothing) merged with min(n, M) items sampled
    uniformly without replacement from the M = n_item - |seen| items outside `seen` (the definition at the top of this file).
    -> (out_p, out_j): canonical CSR, int32."""
    seed, row0, n_item, n = int(seed), int(row0), int(n_item), int(n)
    if not 0 <= seed < 2 ** 64 or row0 < 0 or not 0 <= n_item < 2 ** 31 or n < 1 or (keep_p is None) != (keep_j is None):
        raise ValueError("sample_negatives: bad arguments")
    if n > MAX_NEGATIVES:
        raise NotImplementedError("sample_negatives: n > %d" % MAX_NEGATIVES)
    sp_, sj = np.asarray(seen_p, dtype=np.int64), np.asarray(seen_j, dtype=np.int64)
    n_rows = sp_.size - 1
    if row0 + n_rows > 2 ** 32:
        raise ValueError("sample_negatives: the global row index does not fit 32 bits")
    kp = np.zeros(n_rows + 1, dtype=np.int64) if keep_p is None else np.asarray(keep_p, dtype=np.int64)
    kj = np.zeros(0, dtype=np.int64) if keep_j is None else np.asarray(keep_j, dtype=np.int64)
    rows = []
    for u in range(n_rows):
        seen, keep = sj[sp_[u]:sp_[u + 1]], kj[kp[u]:kp[u + 1]]
        M = n_item - seen.size
        if n >= M:
            ranks = np.arange(max(M, 0), dtype=np.int64)
        else:
            d = min(n, M - n)
            D = first_distinct(seed, row0 + u, M, d)
            ranks = np.sort(D) if 2 * n <= M else np.setdiff1d(np.arange(M, dtype=np.int64), D)
        items = ranks + np.searchsorted(seen - np.arange(seen.size), ranks, side="right")
        rows.append(np.sort(np.concatenate([keep, items])))
    out_p = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    if out_p[-1] >= 2 ** 31:
        raise ValueError("sample_negatives: the output does not fit int32 row pointers")
    out_j = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    return out_p.astype(np.int32), out_j.astype(np.int32)


def mul_hi64(v, W):
    """floor(v W / 2^64) for uint64 arrays (or scalars) v, W: the high half of the 128-bit product, from 32-bit halves in uint64"""
    v, W = np.asarray(v, dtype=np.uint64), np.asarray(W, dtype=np.uint64)
    vl, vh, wl, wh = v & _MASK, v >> _S32, W & _MASK, W >> _S32
    lh, hl = vl * wh, vh * wl
    mid = ((vl * wl) >> _S32) + (lh & _MASK) + (hl & _MASK)       # < 3 * 2^32
    return vh * wh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)


def weights_prefix(w):
    """C[i] = w[0] + ... + w[i] in uint64, for integer weights in [1, 2^32) (a zero is refused)"""
    w = np.asarray(w)
    if w.ndim != 1 or w.dtype.kind not in "iu" or w.size >= 2 ** 31:
        raise ValueError("weights_prefix: the weights are a 1-d integer array of fewer than 2^31 entries")
    if w.size and (int(w.min()) < 1 or int(w.max()) >= 2 ** 32):
        raise ValueError("weights_prefix: a weight outside [1, 2^32)")
    return np.cumsum(w.astype(np.uint64), dtype=np.uint64)


def quantize_weights(v):
    """item weights as the uint32 the weighted stream is defined on.  An integer-dtype array is taken as is and must lie in
    [1, 2^32); float weights -- finite, >= 0, max > 0 -- become max(1, floor(v 2^24 / max(v)))."""
    v = np.asarray(v)
    if v.ndim != 1:
        raise ValueError("quantize_weights: the weights are a 1-d array")
    if v.dtype.kind in "iu":
        if v.size and (int(v.min()) < 1 or int(v.max()) >= 2 ** 32):
            raise ValueError("quantize_weights: an integer weight outside [1, 2^32)")
        return v.astype(np.uint32)
    if v.dtype.kind != "f":
        raise TypeError("quantize_weights: the weights are integers or floats")
    v = v.astype(np.float64)
    if not v.size or not np.isfinite(v).all() or v.min() < 0 or not v.max() > 0:
        raise ValueError("quantize_weights: float weights are finite, >= 0 and have a positive maximum")
    return np.maximum(np.floor(v * float(1 << 24) / v.max()), 1.0).astype(np.uint32)


def popularity_weights(x, power=0.75, smoothing=1.0):
    """(the number of stored entries of every column of the sparse matrix x + smoothing) ** power, quantized"""
    import scipy.sparse as sp
    x = sp.csr_matrix(x)
    cnt = np.bincount(x.indices, minlength=x.shape[1]).astype(np.float64)
    return quantize_weights((cnt + float(smoothing)) ** float(power))


def weighted_draws(seed, g, t0, count, C):
    """the items of the draws t0 .. t0 + count - 1 of global row g under the inclusive weight prefix C -> int64 array"""
    C = np.asarray(C, dtype=np.uint64)
    t = np.arange(t0, t0 + count, dtype=np.uint64)
    c = t >> np.uint64(1)
    counter = np.stack([c & _MASK, np.full_like(c, g), np.full_like(c, STREAM_WEIGHTED_NEGATIVES), c >> _S32], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    o = philox4x32_10(counter, key).astype(np.uint64)
    odd = (t & np.uint64(1)).astype(bool)
    v = (np.where(odd, o[:, 3], o[:, 1]) << _S32) | np.where(odd, o[:, 2], o[:, 0])
    return np.searchsorted(C, mul_hi64(v, C[-1]), side="right").astype(np.int64)


def weighted_budget(n):
    """B(n): the draws a row of the weighted stream may take before it is filled"""
    return 64 * int(n) + 4096


def sample_negatives_weighted(seed, row0, seen_p, seen_j, keep_p, keep_j, n_item, n, w):
    """`sample_negatives` with the negatives drawn in proportion to the integer weights w (n_item of them, every one in
    [1, 2^32); the definition at the top of this file).  -> (out_p, out_j, filled_rows): canonical CSR, int32, and the number of
    rows whose draw budget ended before n distinct admissible items were drawn."""
    seed, row0, n_item, n = int(seed), int(row0), int(n_item), int(n)
    if not 0 <= seed < 2 ** 64 or row0 < 0 or not 0 <= n_item < 2 ** 31 or n < 1 or (keep_p is None) != (keep_j is None):
        raise ValueError("sample_negatives_weighted: bad arguments")
    if n > MAX_NEGATIVES:
        raise NotImplementedError("sample_negatives_weighted: n > %d" % MAX_NEGATIVES)
    C = weights_prefix(w)
    if C.size != n_item:
        raise ValueError("sample_negatives_weighted: one weight per item")
    sp_, sj = np.asarray(seen_p, dtype=np.int64), np.asarray(seen_j, dtype=np.int64)
    n_rows = sp_.size - 1
    if row0 + n_rows > 2 ** 32:
        raise ValueError("sample_negatives_weighted: the global row index does not fit 32 bits")
    kp = np.zeros(n_rows + 1, dtype=np.int64) if keep_p is None else np.asarray(keep_p, dtype=np.int64)
    kj = np.zeros(0, dtype=np.int64) if keep_j is None else np.asarray(keep_j, dtype=np.int64)
    B = weighted_budget(n)
    rows, filled = [], 0
    for u in range(n_rows):
        seen, keep = sj[sp_[u]:sp_[u + 1]], kj[kp[u]:kp[u + 1]]
        M = n_item - seen.size
        if n >= M:
            items = np.setdiff1d(np.arange(n_item, dtype=np.int64), seen)
        else:
            A, t0 = np.zeros(0, dtype=np.int64), 0
            while A.size < n and t0 < B:
                step = min(max(256, 2 * n), B - t0)
                d = weighted_draws(seed, row0 + u, t0, step, C)
                d = np.concatenate([A, d[~np.isin(d, seen)]])
                vals, first = np.unique(d, return_index=True)
                A = d[np.sort(first)][:n]                      # distinct, in the order of their first draw
                t0 += step
            if A.size < n:
                filled += 1
                rest = np.setdiff1d(np.arange(n_item, dtype=np.int64), np.concatenate([seen, A]))
                A = np.concatenate([A, rest[:n - A.size]])
            items = A
        rows.append(np.sort(np.concatenate([keep, items])))
    out_p = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    if out_p[-1] >= 2 ** 31:
        raise ValueError("sample_negatives_weighted: the output does not fit int32 row pointers")
    out_j = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    return out_p.astype(np.int32), out_j.astype(np.int32), filled


def by_keys(by):
    """the order-preserving 64-bit keys of float64 values: larger value <=> larger key, -0.0 just below +0.0 (NaN refused)"""
    by = np.ascontiguousarray(by, dtype=np.float64)
    if np.isnan(by).any():
        raise ValueError("split: NaN in `by`")
    u = by.view(np.uint64)
    return np.where((u >> np.uint64(63)).astype(bool), ~u, u | np.uint64(1 << 63))


def _split_positions(indptr):
    """(row of every entry, its position t in the row) of the row pointers indptr (which may start anywhere)"""
    lens = np.diff(indptr)
    row = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    t = np.arange(int(indptr[-1] - indptr[0]), dtype=np.int64) - (indptr[:-1] - indptr[0])[row]
    return lens, row, t


def split_flags(seed, row0, indptr, test_threshold=None, leave_out=None, min_train=1, by=None):
    """The test flag of every stored entry of the rows with row pointers `indptr` (n_rows + 1 absolute positions; they may be a
    slice of a larger pattern's), global row indices row0, row0 + 1, ...: a bool array of indptr[-1] - indptr[0] entries.
    Exactly one of test_threshold (proportion mode: T = floor(p 2^32)) and leave_out (n >= 1, with min_train >= 0 and, for the
    temporal split, `by`: one float64 per entry of the rows, i.e. the slice [indptr[0], indptr[-1]) of the pattern's) is given."""
    seed, row0 = int(seed), int(row0)
    ip = np.asarray(indptr, dtype=np.int64)
    if ip.ndim != 1 or ip.size < 1 or not 0 <= seed < 2 ** 64 or row0 < 0 or (test_threshold is None) == (leave_out is None):
        raise ValueError("split_flags: bad arguments")
    n_rows = ip.size - 1
    if row0 + n_rows > 2 ** 32:
        raise ValueError("split_flags: the global row index does not fit 32 bits")
    if ip[0] < 0 or (np.diff(ip) < 0).any() or ip[-1] >= 2 ** 31:
        raise ValueError("split_flags: row pointers that are negative, decrease or pass int32")
    lens, row, t = _split_positions(ip)
    g = (row + row0).astype(np.uint64)
    t64 = t.astype(np.uint64)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    if test_threshold is not None:
        T = int(test_threshold)
        if not 0 <= T <= 2 ** 32 or by is not None:
            raise ValueError("split_flags: test_threshold outside [0, 2^32], or `by` in proportion mode")
        counter = np.stack([t64 >> np.uint64(2), g, np.full_like(g, STREAM_SPLIT), np.zeros_like(g)], axis=-1)
        o = philox4x32_10(counter, key)
        word = o[np.arange(t.size), (t & 3)].astype(np.uint64)
        return word < np.uint64(T)
    n, min_train = int(leave_out), int(min_train)
    if n < 1 or min_train < 0:
        raise ValueError("split_flags: leave_out < 1 or min_train < 0")
    if by is not None:
        by = np.asarray(by)
        if by.shape != (t.size,):
            raise ValueError("split_flags: `by` needs one value per entry")
        w = by_keys(by)
    else:
        counter = np.stack([t64 >> np.uint64(1), g, np.full_like(g, STREAM_LEAVE_OUT), np.zeros_like(g)], axis=-1)
        o = philox4x32_10(counter, key).astype(np.uint64)
        odd = (t & 1).astype(bool)
        w = (np.where(odd, o[:, 3], o[:, 1]) << _S32) | np.where(odd, o[:, 2], o[:, 0])
    h = np.minimum(n, np.maximum(lens - min_train, 0))
    # the total order within every row: key descending, position ascending (entries are stored by row, then position)
    order = np.lexsort((t, ~w, row))
    rank = np.empty(t.size, dtype=np.int64)
    rank[order] = t                       # the k-th entry of a row in that order sits at the row's k-th slot
    return rank < h[row]


def split_rows(seed, row0, indptr, indices, test_threshold=None, leave_out=None, min_train=1, by=None):
    """`split_flags` applied: -> (train_p, train_j, train_pos, test_p, test_j, test_pos).  `indices` is the WHOLE pattern's index
    array (indptr holds absolute positions), `by` one value per entry of it or None; *_pos are the absolute source positions of
    the entries, so that values are gathered without being interpreted.  Both outputs are canonical CSR with row pointers from
    0, int32; entries keep their order."""
    ip = np.asarray(indptr, dtype=np.int64)
    idx = np.asarray(indices)
    if by is not None:
        by = np.asarray(by)
        if by.shape != idx.shape:
            raise ValueError("split_rows: `by` needs one value per stored entry")
        by = by[int(ip[0]):int(ip[-1])]
    flags = split_flags(seed, row0, ip, test_threshold, leave_out, min_train, by)
    lens, row, _ = _split_positions(ip)
    pos = np.arange(int(ip[0]), int(ip[-1]), dtype=np.int64)
    out = []
    for f in (~flags, flags):
        cnt = np.bincount(row[f], minlength=lens.size)
        out += [np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), idx[pos[f]].astype(np.int32), pos[f]]
    return tuple(out)
