"""Worst-case inputs for the rank margins of DESIGN 2b, with a CPU-side proof for each that it really is adversarial.

Every MFMA search result is exact only if |recorded rank value - (|v|^2 - 2 q.v)| <= E.  Random data stay one to two
orders below E (the rounding errors of the bf16 split add like a random walk), so a margin that is too small by 2 x
changes nothing a random test looks at.  Here the low mantissa bits are chosen, not drawn: a *victim* whose rank error is
large and positive, K *decoys* whose errors are large and negative, true distances that put the victim first, each of
them alone among 63 far *fillers* in its own 64-slot block.  A margin 2E' < achieved loses the victim.

Pure numpy.  The rank values are emulated in float64 from the operands the kernels multiply (bf16 planes of v and of
-2q, in the plain frame or about a centre mu); the f32 accumulation inside the MFMA is not emulated.  `bound` restates
2E of DESIGN 2b (with the safety factors of query_frame) from the case's own X: nothing is read from the library.

A case is a dict: X (rows in list order), lists (intended list of every row), centroids, q (the adversarial query), Q
(q embedded at ADV_POS among ordinary queries), k, n_probe, radius2 or None, env (the load / search knobs the case
needs), arith, victim / decoys (rows of X), proof.  write_index() puts it on disk through the oracle's shard writer."""
import functools
import importlib.util
import os

import numpy as np

U1 = 1.01 * 2.0 ** -24        # u' of DESIGN 2b
BLOCK, GROUP = 64, 1024
ADV_POS, N_BATCH = 37, 71     # the adversarial query's ragged position among 70 ordinary ones
QUANT = 2.0 ** -22            # centred cases: frame values are multiples of this, so that mu + x is exact in f32
MU = 2.0                      # their common offset (every component): norms about 0 are 5 - 9 x those about mu


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits(a):
    return f32(a).view(np.uint32)


# ---- the bf16 split (mfma_bf16.hpp: bf16_rn, split_pair) on uint32 views ----
def bf16_hi(x):
    x = f32(x)
    b = x.view(np.uint32).astype(np.uint64)
    r = (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32)
    return r.view(np.float32).reshape(x.shape)


def split(x):
    """x = hi + lo + r: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in f32), r the residual; float64"""
    x = f32(x)
    hi = bf16_hi(x)
    lo = bf16_hi(x - hi)
    return hi.astype(np.float64), lo.astype(np.float64), x.astype(np.float64) - hi - lo


def seq_dist(q, V):
    """the reference's distance: one sequential f32 chain acc = acc + (q_d - x_d)^2 per row"""
    q, V = f32(q), f32(V).reshape(-1, len(q))
    acc = np.zeros(V.shape[0], dtype=np.float32)
    for d in range(V.shape[1]):
        t = q[d] - V[:, d]
        acc = acc + t * t
    return acc


# ---- the rank values, float64, in the plain frame (mu None) or about mu ----
def _images(q, V, mu):
    q, V = f32(q), f32(V).reshape(-1, len(q))
    if mu is not None:
        q, V = q - f32(mu), V - f32(mu)          # fl(q - mu), fl(v - mu): what the images are taken from
    return np.float32(-2.0) * q, V                # the query image is that of -2q (exact scaling)


def true_rank(q, V, mu=None):
    A, Vf = _images(q, V, mu)
    Vd = Vf.astype(np.float64)
    return (Vd * Vd).sum(axis=1) + Vd @ A.astype(np.float64)


def rank_bf16x3(q, V, mu=None):
    """hi.hi + hi.lo + lo.hi"""
    A, Vf = _images(q, V, mu)
    Ah, Al, _ = split(A)
    Vh, Vl, _ = split(Vf)
    Vd = Vf.astype(np.float64)
    return (Vd * Vd).sum(axis=1) + Vh @ Ah + Vl @ Ah + Vh @ Al


def rank_hi_lists(q, V, mu=None):
    """lists hi only, queries hi + lo (rank_mode 4 / 6, VI_RANK_APPROX=1)"""
    A, Vf = _images(q, V, mu)
    Ah, Al, _ = split(A)
    Vh, _, _ = split(Vf)
    Vd = Vf.astype(np.float64)
    return (Vd * Vd).sum(axis=1) + Vh @ (Ah + Al)


def rank_hi_both(q, V, mu=None):
    """lists and queries hi only (VI_RANK_APPROX=2)"""
    A, Vf = _images(q, V, mu)
    Ah, _, _ = split(A)
    Vh, _, _ = split(Vf)
    Vd = Vf.astype(np.float64)
    return (Vd * Vd).sum(axis=1) + Vh @ Ah


def rank_int8(q, V, mu=None):
    """2 ceil(|v'|^2 / 2) - 2 q'.v' about 127 (integers)"""
    qi = np.asarray(q, dtype=np.int64) - 127
    Vi = np.asarray(V, dtype=np.int64).reshape(-1, len(qi)) - 127
    n = (Vi * Vi).sum(axis=1)
    return (2 * ((n + 1) // 2) - 2 * (Vi @ qi)).astype(np.float64)


def true_rank_int8(q, V):
    qi = np.asarray(q, dtype=np.int64) - 127
    Vi = np.asarray(V, dtype=np.int64).reshape(-1, len(qi)) - 127
    return ((Vi * Vi).sum(axis=1) - 2 * (Vi @ qi)).astype(np.float64)


RANK = {"bf16x3": rank_bf16x3, "hi_lists": rank_hi_lists, "hi_both": rank_hi_both, "int8": rank_int8}


# ---- 2E of DESIGN 2b, restated ----
def bound_2E(arith, q, X, mu=None, lolo=1.01 * 2.0 ** -15, with_qres=True, trunc_scale=1.0):
    """E = e (|q|^2 (1 + gamma) + 2 max|v|^2), e = (3D + 2) 2u' + lolo (+ 6u' about a centre), for the hi-plane forms plus
    1.02 (2 |q| rho_max (1 + 2^-8) + |(-2q) - hi(-2q)| max|v|); int8: E = 1.  max|v|, rho_max from X itself, in the frame
    the rank values live in.  lolo = 3 * 2^-18 is the round-2 budget."""
    if arith == "int8":
        return 2.0
    D = X.shape[1]
    A, Xf = _images(q, X, mu)
    Xd = Xf.astype(np.float64)
    qn = float((A.astype(np.float64) ** 2).sum()) / 4.0
    xmax2 = float((Xd * Xd).sum(axis=1).max())
    gamma = (D + 2.0) * U1
    e = (3.0 * D + 2.0) * 2.0 * U1 + lolo + (6.0 * U1 if mu is not None else 0.0)
    E = e * (qn * (1.0 + gamma) + 2.0 * xmax2)
    if arith in ("hi_lists", "hi_both"):
        R = Xd - bf16_hi(Xf).astype(np.float64)
        rho = float(np.sqrt((R * R).sum(axis=1).max()))
        t = 2.0 * np.sqrt(qn) * rho * (1.0 + 0.00391) * trunc_scale
        if arith == "hi_both" and with_qres:
            qr = A.astype(np.float64) - bf16_hi(A).astype(np.float64)
            t += float(np.sqrt((qr * qr).sum())) * np.sqrt(xmax2)
        E += 1.02 * t
    return 2.0 * E


def load_stats(X, mu=None):
    """(max|v|, max|v - hi(v)|) over the stored vectors, in the centred frame where centred"""
    Xf = f32(X) if mu is None else f32(X) - f32(mu)
    Xd = Xf.astype(np.float64)
    R = Xd - bf16_hi(Xf).astype(np.float64)
    return float(np.sqrt((Xd * Xd).sum(axis=1).max())), float(np.sqrt((R * R).sum(axis=1).max()))


def centring_rule(X):
    """the load-time centring rule restated (images about the mean): mu = f32(mean of the stored vectors), and
    the images are taken about it when that at least halves mean|v|^2 + 2 max|v|^2 -> (mu, picked)"""
    Xd = f32(X).astype(np.float64)
    mu = f32(Xd.sum(axis=0) / len(Xd))
    raw = (Xd * Xd).sum(axis=1)
    Xc = (f32(X) - mu).astype(np.float64)
    mean_c = max(0.0, raw.mean() - float((mu.astype(np.float64) ** 2).sum()))
    return mu, bool(mean_c + 2.0 * (Xc * Xc).sum(axis=1).max() < 0.5 * (raw.mean() + 2.0 * raw.max()))


# ---- fillers: far from every adversarial query, norm below the victim's ----
def _quantise(m):
    return np.round(m / QUANT) * QUANT


def balanced_fillers(rng, n, D):
    """|x_d| in [0.5, 1), exactly D/2 negative components per row: |f|^2 < D, and |f|^2 - 2 q.f >= 0.125 D for q = c (1..1),
    c <= 1.  Returned in pairs (f, -f): the rows sum to zero exactly, so a centre mu stays the mean."""
    half = (n + 1) // 2
    mag = _quantise(0.5 + 0.4999 * rng.random((half, D)))
    sign = np.ones((half, D))
    sign[:, : D // 2] = -1.0
    sign = rng.permuted(sign, axis=1)
    F = mag * sign
    out = np.empty((2 * half, D))
    out[0::2], out[1::2] = F, -F
    return out


def negative_fillers(rng, n, D):
    """every component in [-0.9, -0.7]: |f|^2 <= 0.81 D and |f|^2 - 2 q.f >= 1.19 D for q = 0.5 (1..1)"""
    return -(0.7 + 0.2 * rng.random((n, D)))


# ---- where victim and decoys sit in the adversarial list ----
def placement(K, spread):
    """(blocks of the list, victim block, decoy blocks).  near: all decoys inside the first 1024-vector group, the victim
    in the second; far: decoys 17 blocks (1088 positions) apart.  The victim comes after the decoys in candidate order."""
    if K == 1:
        return 5, 3, [1]
    if spread == "near":
        return 20, 17, list(range(1, K + 1))
    return 17 * K + 4, 17 * K + 2, [17 * i for i in range(K)]


def slot_of(block):
    return (11 * block + 5) % BLOCK


def _free_dim_push(q, vec, j, target_bits, at_least):
    """vec with component j (a dimension where q is 0) set to the smallest t >= 0 whose distance bits are >= target
    (at_least) or the largest whose bits are <= target; the distance is monotone in t"""
    def dist_bits(tb):
        c = vec.copy()
        c[j] = np.uint32(tb).view(np.float32)
        return int(bits(seq_dist(q, c[None]))[0])
    lo, hi = 0, 0x3F800000          # t in [0, 1]
    if at_least:
        assert dist_bits(hi) >= target_bits
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if dist_bits(mid) >= target_bits else (mid + 1, hi)
    else:
        assert dist_bits(0) <= target_bits
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if dist_bits(mid) <= target_bits else (lo, mid - 1)
    c = vec.copy()
    c[j] = np.uint32(lo).view(np.float32)
    return c


def order_by_free_dim(q, vic, dec, j, gap):
    """the f32 distance of dec becomes `gap` ulps more than vic's, by the free dimension j of one of them"""
    dv, dw = int(bits(seq_dist(q, vic[None]))[0]), int(bits(seq_dist(q, dec[None]))[0])
    if dw - dv >= gap:
        vic = _free_dim_push(q, vic, j, dw - gap, at_least=False)
    else:
        dec = _free_dim_push(q, dec, j, dv + gap, at_least=True)
    return vic, dec


# ---- the scalar patterns ----
def straddle(quant):
    """one step below and above the bf16 rounding tie 1 + 2^-8: hi planes 1 and 1 + 2^-7"""
    return 1.0 + 2.0 ** -8 - quant, 1.0 + 2.0 ** -8 + quant


@functools.lru_cache(maxsize=None)
def bf16x3_patterns(step_bits):
    """(a, x_victim, x_decoy) about 1: the query scalar a and two stored scalars whose bf16 x 3 rank errors
    -(A x - (Ah xh + Ah xl + Al xh)), A = -2a, are most positive and most negative, with a one step off the midpoint of
    the two on the victim's side, so that the victim is the nearer one by a hair in every dimension.  Searched over the
    low 16 mantissa bits of values in [1, 1 + 2^-7), in steps of 2^step_bits ulps."""
    unit = 1 << step_bits
    js = np.unique((np.arange(0, 1 << 16, 37) // (2 * unit)) * (2 * unit))     # even multiples: the midpoint is on the grid
    x = 1.0 + js.astype(np.float64) * 2.0 ** -23
    X1, X2 = np.meshgrid(x, x, indexing="ij")
    Am = f32(-(X1 + X2))                                                        # A = -2a, a the midpoint
    Ah, Al, _ = split(Am)

    def err(xv):
        xh, xl, _ = split(f32(xv))
        return (Ah * xh + Ah * xl + Al * xh) - Am.astype(np.float64) * xv

    gain = err(X1) - err(X2)
    i, j = np.unravel_index(np.argmax(gain), gain.shape)
    x1, x2 = x[i], x[j]
    a = (x1 + x2) / 2.0 + (unit * 2.0 ** -23 if x1 > x2 else -unit * 2.0 ** -23)
    assert x1 != x2 and np.float32(a) == a and abs(a - x1) < abs(a - x2)
    return float(a), float(x1), float(x2)


# ---- the constructors ----
def _assemble(name, D, K, spread, q, vic, dec, arith, env, filler_kind, mu=None, seed=0, radius=False, k=None,
              extra=None):
    """list 0: victim and K copies of the decoy alone in their blocks among fillers; lists 1, 2: fillers and, about a
    centre, the mirror images that keep the mean on mu.  Frame values in, stored values (mu added) out."""
    rng = np.random.default_rng(1000 * D + 10 * K + seed)
    nb, vb, dbs = placement(K, spread)
    len0 = nb * BLOCK - 23                                   # the last block is ragged
    nfill = len0 - (K + 1) + 2 * 96
    nfill += nfill & 1
    F = balanced_fillers(rng, nfill, D) if filler_kind == "balanced" else negative_fillers(rng, nfill, D)
    rows = np.empty((len0, D))
    special = {vb * BLOCK + slot_of(vb): vic}
    for b in dbs:
        special[b * BLOCK + slot_of(b)] = dec
    gaps = [p for p in range(len0) if p not in special]
    rows[gaps] = F[: len(gaps)]
    for p, v in special.items():
        rows[p] = v
    rest = F[len(gaps):]
    if filler_kind == "balanced":                            # mirror images of the special rows: the frame sum stays 0
        rest = np.concatenate([rest, -vic[None], np.repeat(-dec[None], K, axis=0)])
    half = len(rest) // 2
    Xf = np.concatenate([rows, rest[:half], rest[half:]])
    lists = np.concatenate([np.zeros(len0, int), np.ones(half, int), np.full(len(rest) - half, 2, int)])
    cents = np.stack([np.asarray(dec, dtype=np.float64), rest[:half].mean(axis=0) - 0.25, rest[half:].mean(axis=0) + 0.25])
    ordinary = F[rng.integers(0, len(F), N_BATCH - 1)] * (1.0 + 0.01 * rng.standard_normal((N_BATCH - 1, D)))
    Qf = np.concatenate([ordinary[:ADV_POS], np.asarray(q)[None], ordinary[ADV_POS:]])
    off = 0.0 if mu is None else MU
    X, Q, C = f32(Xf + off), f32(Qf + off), f32(cents + off)
    Q[ADV_POS] = f32(np.asarray(q) + off)
    muv = None if mu is None else np.full(D, MU, dtype=np.float32)
    if muv is not None:                                      # the frame values survive the translation, and mu is the mean
        assert np.array_equal((X - muv).astype(np.float64), Xf) and np.array_equal((Q[ADV_POS] - muv).astype(np.float64), q)
        assert np.array_equal(X.astype(np.float64).sum(axis=0) / len(X), muv.astype(np.float64))
    else:
        assert np.array_equal(X[list(special)].astype(np.float64), np.stack(list(special.values())))
    victim = vb * BLOCK + slot_of(vb)
    decoys = [b * BLOCK + slot_of(b) for b in dbs]
    case = dict(name=name, D=D, K=K, X=X, lists=lists, centroids=C, q=Q[ADV_POS].copy(), Q=Q, k=k or K, n_probe=2,
                radius2=None, env=dict(env), arith=arith, mu=muv, victim=victim, decoys=decoys, integer=False)
    case["proof"] = prove(case, extra)
    if muv is not None:      # the rule picks this centre on its own, and the centre it computes is mu to the bit
        mu_rule, picked = centring_rule(X)
        case["proof"].update(centre_picked_by_rule=picked, centre_is_mu=bool(np.array_equal(bits(mu_rule), bits(muv))))
    if radius:
        case["radius2"] = float(case["proof"]["victim_dist"])
    return case


def prove(case, extra=None):
    X, q, mu, arith = case["X"], case["q"], case["mu"], case["arith"]
    v, w = case["victim"], case["decoys"][-1]                # (the decoys are copies: the K-th is any of them)
    if arith == "int8":
        rec, tru = rank_int8(q, X[[v, w]]), true_rank_int8(q, X[[v, w]])
    else:
        rec, tru = RANK[arith](q, X[[v, w]], mu), true_rank(q, X[[v, w]], mu)
    achieved = float((rec[0] - tru[0]) - (rec[1] - tru[1]))
    bound = bound_2E(arith, q, X, mu)
    d = seq_dist(q, X)
    others = np.ones(len(X), bool)
    others[[v] + case["decoys"]] = False
    p = dict(achieved=achieved, bound=bound, strength=achieved / bound, e_plus=float(rec[0] - tru[0]), e_minus=float(tru[1] - rec[1]),
             victim_dist=np.float32(d[v]), decoy_dist=np.float32(d[w]), victim_strictly_nearer=bool(d[v] < d[w]),
             nearest_filler_dist=np.float32(d[others].min()),
             # what the select sees: the victim's recorded value against the decoys' (the K-th smallest sub-block minimum)
             recorded_gap=float(rec[0] - rec[1]),
             max_norm_row_is_special=bool(int(np.argmax((X.astype(np.float64) ** 2).sum(axis=1))) in [v] + case["decoys"])
             if mu is None else None)
    if extra:
        p.update(extra(case, p))
    return p


def case_a(D, K, spread="near", centred=False, radius=False):
    """hi planes of the lists only: q = (1/2)(1..1), victim one step below the tie 1 + 2^-8, decoy one step above.  The
    lower vector is the nearer one; the hi-plane rank prefers the upper one by 2 (2 |q| rho)."""
    lo, up = straddle(QUANT if centred else 2.0 ** -23)
    name = f"A{'c' if centred else ''}{'r' if radius else ''}-D{D}-K{K}{'-' + spread if K > 1 else ''}"
    return _assemble(name, D, K, spread, np.full(D, 0.5), np.full(D, lo), np.full(D, up), "hi_lists",
                     {"VI_RANK_APPROX": "1", "VI_CENTER": "1" if centred else "0"}, "balanced",
                     mu=MU if centred else None, radius=radius, k=1 if radius else None)


def case_b(D, K, spread="near"):
    """hi planes of lists and queries: on D - 2 dimensions the victim is (+lo.., -up..) and the decoy its negative, the
    query image -2q straddles the same tie with the sign pattern of the victim, so that both the query's own residual
    and the lists' act on victim and decoy with opposite signs; q.v is about 0 and the two true distances agree to a few
    ulps, settled by a free dimension (q = 0 there)."""
    P, h = D - 2, (D - 2) // 2
    lo, up = straddle(2.0 ** -23)
    vic, q = np.zeros(D), np.zeros(D)
    vic[:h], vic[h:P] = lo, -up
    q[:h], q[h:P] = lo / 2.0, up / 2.0        # -2q = -(tie - step) where v > 0, -(tie + step) where v < 0
    vic, dec = order_by_free_dim(f32(q), f32(vic), f32(-vic), D - 2, gap=1)

    def extra(case, p):
        without = bound_2E("hi_both", case["q"], case["X"], None, with_qres=False)
        return dict(bound_without_query_residual=without, needs_query_residual=bool(p["achieved"] > without))
    return _assemble(f"B-D{D}-K{K}{'-' + spread if K > 1 else ''}", D, K, spread, q, vic.astype(np.float64),
                     dec.astype(np.float64), "hi_both", {"VI_RANK_APPROX": "2", "VI_CENTER": "0"}, "negative", extra=extra)


def c_vectors(D, centred=False, gap=1):
    """bf16 x 3: q = a (1..1), victim x1 (1..1), decoy x2 (1..1) with coherent lo.lo and residual patterns; a sits one
    step off their midpoint, which orders the two f32 distances without a free dimension"""
    a, x1, x2 = bf16x3_patterns(1 if centred else 0)
    q, vic, dec = np.full(D, a), np.full(D, x1), np.full(D, x2)
    dv, dw = bits(seq_dist(f32(q), f32(vic)[None]))[0], bits(seq_dist(f32(q), f32(dec)[None]))[0]
    assert int(dw) - int(dv) >= gap, (dv, dw)
    return q, vic, dec


def round2_extra(case, p):
    r2 = bound_2E(case["arith"], case["q"], case["X"], case["mu"], lolo=3.0 * 2.0 ** -18)
    return dict(bound_round2=r2, strength_round2=p["achieved"] / r2)


def case_c(D, K, spread="near", centred=False, radius=False):
    q, vic, dec = c_vectors(D, centred)
    name = f"C{'c' if centred else ''}{'r' if radius else ''}-D{D}-K{K}{'-' + spread if K > 1 else ''}"
    return _assemble(name, D, K, spread, q, vic, dec, "bf16x3", {"VI_RANK_APPROX": "0", "VI_CENTER": "1" if centred else "0"},
                     "balanced", mu=MU if centred else None, radius=radius, k=1 if radius else None, extra=round2_extra)


def case_e(K, spread="near", radius=False):
    """int8 ranks, D = 128, about 127: q' = (2, 0..), victim v' = (1, 0..) at distance 1 with |v'|^2 odd (record m' + 1 =
    -2), decoy w' = (2, 1, 1, 0..) at distance 2 with |w'|^2 even (record m' = -2).  m' and |v'|^2 have the same parity, so
    two vectors at the SAME distance cannot differ in the parity of their norms: in a top-k the records order as the
    distances do and e_abs = 0 loses nothing (proof: parity_note).  The radius select is where the unit counts: with
    radius2 = 1 the victim's record -2 lies above radius2 - |q'|^2 = -3.
    So only the radius case (Er) is adversarial for e_abs.  The top-k cases (E-K1, E-K10-near) pass for ANY e_abs: their
    records tie, the victim's sub-block is re-evaluated with e_abs = 0 too.  They are parity runs of the int8 route on tied
    records, not margin coverage; their `strength` 0.5 only says e+ = 1 of 2E = 2."""
    D = 128
    rng = np.random.default_rng(7 + K + (100 if radius else 0))
    nb, vb, dbs = placement(K, spread)
    len0 = nb * BLOCK - 23
    n = len0 + 2 * 96
    F = 127 + rng.integers(20, 41, size=(n, D)) * rng.choice([-1, 1], size=(n, D))
    q = np.full(D, 127)
    q[0] = 129
    vic, dec = np.full(D, 127), np.full(D, 127)
    vic[0] = 128
    dec[0], dec[1], dec[2] = 129, 128, 128
    X = F.copy()
    victim = vb * BLOCK + slot_of(vb)
    decoys = [b * BLOCK + slot_of(b) for b in dbs]
    X[victim] = vic
    X[decoys] = dec
    lists = np.concatenate([np.zeros(len0, int), np.ones(96, int), np.full(96, 2, int)])
    C = np.stack([np.full(D, 127.0), X[len0:len0 + 96].mean(axis=0), X[len0 + 96:].mean(axis=0)])
    ordinary = np.clip(F[rng.integers(0, n, N_BATCH - 1)] + rng.integers(-3, 4, size=(N_BATCH - 1, D)), 0, 254)
    Q = f32(np.concatenate([ordinary[:ADV_POS], q[None], ordinary[ADV_POS:]]))
    case = dict(name=f"E{'r' if radius else ''}-K{K}{'-' + spread if K > 1 else ''}", D=D, K=K, X=f32(X), lists=lists, centroids=f32(C),
                q=f32(q), Q=Q, k=1 if radius else K, n_probe=2, radius2=1.0 if radius else None, env={"VI_CENTER": "0"}, arith="int8",
                mu=None, victim=victim, decoys=decoys, integer=True)

    def extra(case, p):
        rec = rank_int8(case["q"], case["X"][[victim, decoys[-1]]])
        tru = true_rank_int8(case["q"], case["X"][[victim, decoys[-1]]])
        qn = float(((case["q"].astype(np.float64) - 127) ** 2).sum())
        gamma3 = 3.0 * (D + 2) * U1 * (max(tru[1] + qn, 0.0) + 1.0)
        return dict(records=rec.tolist(), true=tru.tolist(), victim_norm_odd=bool(int(((case["X"][victim].astype(np.int64) - 127) ** 2).sum()) % 2 == 1),
                    decoy_norm_even=bool(int(((case["X"][decoys[-1]].astype(np.int64) - 127) ** 2).sum()) % 2 == 0),
                    gamma_term=gamma3, radius_frame=1.0 - qn,
                    parity_note="m' = |v'|^2 - 2 q'.v' has the parity of |v'|^2 and the record is 2 ceil(m'/2): monotone in m'")
    case["proof"] = prove(case, extra)
    return case


# ---- G: the coarse step on the matrix cores; H: the k-means assign tiers ----
@functools.lru_cache(maxsize=None)
def coarse_table(D=16, nq=256, n_copies=200):
    """1088 centroids, one list of one row (the centroid) each; centroids 209 and 616 are the bf16 x 3 pair.  nq queries:
    copies of the adversarial query at ragged positions among ordinary ones.  D = 4 is the table on which the round-2
    budget is exceeded (strength_round2 > 1); at D = 16 the accumulation term already hides it."""
    k = 1088
    rng = np.random.default_rng(16 + D)
    q, vic, dec = c_vectors(D, gap=16)           # (a wider gap: the k-means oracle sums in another order)
    C = balanced_fillers(rng, k, D)[:k]
    victim, decoy = 3 * BLOCK + 17, 9 * BLOCK + 40
    C[victim], C[decoy] = vic, dec
    Q = C[rng.integers(0, k, nq)] * (1.0 + 0.02 * rng.standard_normal((nq, D)))
    adv = np.sort(rng.choice(nq, n_copies, replace=False))
    Q[adv] = q
    case = dict(name=f"G-D{D}", D=D, K=1, X=f32(C), lists=np.arange(k), centroids=f32(C), q=f32(q), Q=f32(Q), adv_rows=adv,
                k=1, n_probe=1, radius2=None, env={"VI_RANK_APPROX": "0", "VI_CENTER": "0"}, arith="bf16x3", mu=None,
                victim=victim, decoys=[decoy], integer=False)
    case["proof"] = prove(case, round2_extra)
    return case


def assign_bound(x, C, lolo=1.01 * 2.0 ** -15):
    """the margin of the bf16 x 3 assign tier (assign_mfma.hip): 2 (e + g) |x|^2 + 2 (2e + g) max|c|^2"""
    D = C.shape[1]
    e = (3.0 * D + 2.0) * 2.0 * U1 + lolo
    g = (D / 8.0 + 8.0) * U1 * 2.0
    x2 = float((f32(x).astype(np.float64) ** 2).sum())
    cmax = float((f32(C).astype(np.float64) ** 2).sum(axis=1).max())
    return 2.0 * (e + g) * x2 + 2.0 * (2.0 * e + g) * cmax


@functools.lru_cache(maxsize=None)
def assign_case(D=4, n=1500, n_copies=300):
    """points against the table of G: the copies of the adversarial point are nearest to `victim`, the bf16 x 3 tier
    ranks `decoy` ahead of it by `achieved`"""
    g = coarse_table(D)
    rng = np.random.default_rng(17 + D)
    X = rng.standard_normal((n, D)) * 0.8
    adv = np.sort(rng.choice(n, n_copies, replace=False))
    X[adv] = g["q"]
    bound = assign_bound(g["q"], g["centroids"])
    proof = dict(achieved=g["proof"]["achieved"], bound=bound, strength=g["proof"]["achieved"] / bound)
    return dict(name=f"H-D{D}" + (f"-n{n}" if n != 1500 else ""), X=f32(X), centroids=g["centroids"], adv_rows=adv, victim=g["victim"], decoy=g["decoys"][0],
                proof=proof)


def assign_sweep_bound(x, C):
    """the margin of the hi-only candidate sweep (assign_mfma.hip): 2 (e_tr + e_acc + g) |x|^2 + 2 (e_tr + 2 e_acc + g) max|c|^2"""
    D = C.shape[1]
    e_tr = 2.0 ** -7 * (1.0 + 2.0 ** -9) * 1.01
    e_acc = (D + 2.0) * 2.0 * U1
    g = (D / 8.0 + 8.0) * U1 * 2.0
    x2 = float((f32(x).astype(np.float64) ** 2).sum())
    cmax = float((f32(C).astype(np.float64) ** 2).sum(axis=1).max())
    return 2.0 * (e_tr + e_acc + g) * x2 + 2.0 * (e_tr + 2.0 * e_acc + g) * cmax


@functools.lru_cache(maxsize=None)
def assign_sweep_case(D=16, k=8192, n=1500, n_copies=300):
    """the candidate sweep (first assign tier from 8192 centroids on) ranks hi(x).hi(c): the geometry of case B with
    |x| = |c| (where 2^-6 |x||c| = 2^-7 (|x|^2 + |c|^2)): victim (+lo.., -up..), decoy its negative, the point straddling
    the same tie with the victim's sign pattern"""
    P, h = D - 2, (D - 2) // 2
    lo, up = straddle(2.0 ** -23)
    vic, x = np.zeros(D), np.zeros(D)
    vic[:h], vic[h:P] = lo, -up
    x[:h], x[h:P] = lo, up
    vic, dec = order_by_free_dim(f32(x), f32(vic), f32(-vic), D - 2, gap=16)
    rng = np.random.default_rng(8192)
    C = negative_fillers(rng, k, D)
    victim, decoy = 70 * BLOCK + 9, 100 * BLOCK + 33
    C[victim], C[decoy] = vic, dec
    X = rng.standard_normal((n, D)) * 0.8
    adv = np.sort(rng.choice(n, n_copies, replace=False))
    X[adv] = x
    X, C = f32(X), f32(C)
    rec, tru = rank_hi_both(x, C[[victim, decoy]]), true_rank(x, C[[victim, decoy]])
    achieved = float((rec[0] - tru[0]) - (rec[1] - tru[1]))
    bound = assign_sweep_bound(x, C)
    return dict(name=f"H-sweep-D{D}", X=X, centroids=C, adv_rows=adv, victim=victim, decoy=decoy,
                proof=dict(achieved=achieved, bound=bound, strength=achieved / bound))


# ---- every list-search case, by name ----
def _list_cases():
    out = []
    for D in (16, 128):
        out += [lambda D=D: case_a(D, 1), lambda D=D: case_a(D, 10, "near"), lambda D=D: case_a(D, 10, "far")]
    out += [lambda: case_b(16, 1), lambda: case_b(16, 10, "near"), lambda: case_b(16, 10, "far"), lambda: case_b(128, 1),
            lambda: case_b(128, 10, "near")]
    out += [lambda: case_c(4, 1), lambda: case_c(16, 1), lambda: case_c(16, 10, "near"), lambda: case_c(132, 1)]
    out += [lambda: case_a(16, 1, centred=True), lambda: case_a(16, 10, "near", centred=True), lambda: case_c(16, 1, centred=True)]
    out += [lambda: case_e(1), lambda: case_e(10, "near")]
    out += [lambda: case_a(16, 1, radius=True), lambda: case_c(16, 1, radius=True), lambda: case_e(1, radius=True)]
    return out


LIST_CASE_NAMES = ["A-D16-K1", "A-D16-K10-near", "A-D16-K10-far", "A-D128-K1", "A-D128-K10-near", "A-D128-K10-far",
                   "B-D16-K1", "B-D16-K10-near", "B-D16-K10-far", "B-D128-K1", "B-D128-K10-near", "C-D4-K1", "C-D16-K1", "C-D16-K10-near", "C-D132-K1",
                   "Ac-D16-K1", "Ac-D16-K10-near", "Cc-D16-K1", "E-K1", "E-K10-near", "Ar-D16-K1", "Cr-D16-K1", "Er-K1"]


@functools.lru_cache(maxsize=None)
def list_case(name):
    case = _list_cases()[LIST_CASE_NAMES.index(name)]()
    assert case["name"] == name, (case["name"], name)
    return case


# ---- on disk: index.bin as the golden generator writes it, one shard through the oracle's writer ----
def _index_bin():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py")
    spec = importlib.util.spec_from_file_location("make_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.index_bin


def write_index(case, root):
    """-> (index_dir, shards_dir).  External id = row of X.  The centroids are stored exactly as constructed."""
    import oracle_lib as O
    idx, sh = os.path.join(str(root), "index"), os.path.join(str(root), "shards")
    os.makedirs(idx, exist_ok=True)
    os.makedirs(sh, exist_ok=True)
    C, D = case["centroids"], case["D"]
    nl = len(C)
    with open(os.path.join(idx, "index.bin"), "wb") as f:
        f.write(_index_bin()(C, [0] * nl, D))
    lists = []
    for l in range(nl):
        rows = np.nonzero(case["lists"] == l)[0].astype(np.uint64)
        lists.append((rows, rows, np.full(len(rows), 1_700_000_000, dtype=np.uint64), case["X"][rows.astype(np.int64)]))
    assert O.shard_save(sh, 0, D, np.arange(nl, dtype=np.uint64), C, lists) == O.ORC_OK
    return idx, sh
