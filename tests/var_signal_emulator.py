"""The two-level tiling of kernels_var_signal.hip in numpy f32 (no FMA): tiles of 64 samples, groups of 64 tiles.

  tails    tile-local tails (E1, P1, E2, G, P2) of every tile, as tile_tails forms them
  scan     per group a Kogge-Stone scan across the 64 lanes: the prefix of (E1, P1), the suffix of the whole tuple; from them a
           lane's map  c_l = a + b c_g,  d_l = A + B c_g + C d_g  and the group's aggregate
  carry    the serial recurrences over groups: c forward, d backward with the G c term
  final    every tile's recurrences rerun from (c_l, d_l)
`compose` is the monoid of the tuples; `serial` is the plain loop in any type, the yardstick."""
import numpy as np

CAUSAL, ANTICAUSAL, PAIR = 0, 1, 2
T = 64          # samples of a tile
L = 64          # tiles of a group
f32 = np.float32


def serial(x, w, causal, dtype):
    """one scan of the 1-D signal x with the weights w (w[0] never read), in `dtype`"""
    n = len(x)
    v = np.asarray(x, dtype=dtype)
    wt = np.zeros(n + 1, dtype=dtype)
    wt[1:n] = np.asarray(w, dtype=dtype)[1:n]
    y = np.empty(n, dtype=dtype)
    one = dtype(1)
    acc = dtype(0)
    for i in (range(n) if causal else range(n - 1, -1, -1)):
        wi = wt[i] if causal else wt[i + 1]
        acc = (one - wi) * v[i] + wi * acc
        y[i] = acc
    return y


def serial_stage(x, w, mode, dtype):
    v = x
    if mode != ANTICAUSAL:
        v = serial(v, w, True, dtype)
    if mode != CAUSAL:
        v = serial(v, w, False, dtype)
    return v


def compose(A, B):
    """sub-line A followed on its right by B; tuples (E1, P1, E2, G, P2) of scalars or arrays, in their own type"""
    e1a, p1a, e2a, ga, p2a = A
    e1b, p1b, e2b, gb, p2b = B
    return (e1b + p1b * e1a, p1b * p1a, e2a + p2a * (e2b + gb * e1a), ga + (p2a * gb) * p1a, p2a * p2b)


def identity(shape=(), dtype=f32):
    z, o = np.zeros(shape, dtype), np.ones(shape, dtype)
    return (z, o, z.copy(), z.copy(), o.copy())


def _tiles(x, w):
    """(x as (M, 64), masked weights as (M, 65)), M a multiple of 64: samples and weights past the end, and weight 0, are 0"""
    n = len(x)
    m = -(-n // T)
    m = -(-m // L) * L
    xp = np.zeros(m * T, f32)
    xp[:n] = x
    wp = np.zeros(m * T + 1, f32)
    wp[1:n] = np.asarray(w, f32)[1:n]
    idx = np.arange(m)[:, None] * T + np.arange(T + 1)[None, :]
    return xp.reshape(m, T), wp[idx]


def tile_tails(xt, wt):
    m = xt.shape[0]
    one = f32(1)
    p = wt[:, 0].copy()
    qq = np.ones(m, f32)
    g = np.zeros(m, f32)
    for i in range(T):
        if i > 0:
            p = p * wt[:, i]
            qq = qq * wt[:, i]
        g = g + (qq * (one - wt[:, i + 1])) * p
    p1, p2 = p, qq * wt[:, T]
    u = np.empty_like(xt)
    prev = np.zeros(m, f32)
    for i in range(T):
        prev = (one - wt[:, i]) * xt[:, i] + wt[:, i] * prev
        u[:, i] = prev
    e1 = prev
    return u, e1, p1, g, p2


def anticausal_tail(v, wt):
    one = f32(1)
    acc = np.zeros(v.shape[0], f32)
    for i in range(T - 1, -1, -1):
        acc = (one - wt[:, i + 1]) * v[:, i] + wt[:, i + 1] * acc
    return acc


def tiled_stage(x, w, mode):
    """one stage (CAUSAL, ANTICAUSAL or PAIR) of the signal x by the two-level scheme, f32 throughout"""
    n = len(x)
    xt, wt = _tiles(np.asarray(x, f32), w)
    m = xt.shape[0]
    G = m // L
    u, e1, p1, g, p2 = tile_tails(xt, wt)
    e2 = anticausal_tail(u if mode == PAIR else xt, wt)
    if mode == CAUSAL:
        e2, g, p2 = np.zeros(m, f32), np.zeros(m, f32), np.ones(m, f32)
    if mode == ANTICAUSAL:
        e1, p1, g = np.zeros(m, f32), np.ones(m, f32), np.zeros(m, f32)
    if mode != PAIR:
        g = np.zeros(m, f32)
    own = tuple(a.reshape(G, L) for a in (e1, p1, e2, g, p2))
    lane = np.arange(L)[None, :]
    # inclusive prefix across the lanes (only E1 and P1 of it are used)
    pre = own
    k = 1
    while k < L:
        up = tuple(np.roll(a, k, axis=1) for a in pre)
        nxt = compose(up, pre)
        pre = tuple(np.where(lane >= k, b, a) for a, b in zip(pre, nxt))
        k *= 2
    # inclusive suffix
    suf = own
    k = 1
    while k < L:
        dn = tuple(np.roll(a, -k, axis=1) for a in suf)
        nxt = compose(suf, dn)
        suf = tuple(np.where(lane + k < L, b, a) for a, b in zip(suf, nxt))
        k *= 2
    ident = identity((G, 1))
    a_l = np.concatenate([ident[0], pre[0][:, :-1]], axis=1)
    b_l = np.concatenate([ident[1], pre[1][:, :-1]], axis=1)
    S = tuple(np.concatenate([s[:, 1:], i], axis=1) for s, i in zip(suf, ident))
    A_l = S[2] + S[3] * pre[0]
    B_l = S[3] * pre[1]
    C_l = S[4]
    whole = tuple(s[:, 0] for s in suf)
    if mode == CAUSAL:
        whole = tuple(p[:, -1] for p in pre)
    # carries over groups
    c_g = np.zeros(G, f32)
    d_g = np.zeros(G, f32)
    c = f32(0)
    for q in range(G):
        c_g[q] = c
        c = whole[0][q] + whole[1][q] * c
    d = f32(0)
    for q in range(G - 1, -1, -1):
        d_g[q] = d
        d = (whole[2][q] + whole[3][q] * c_g[q]) + whole[4][q] * d
    c_l = (a_l + b_l * c_g[:, None]).reshape(m).astype(f32)
    d_l = ((A_l + B_l * c_g[:, None]) + C_l * d_g[:, None]).reshape(m).astype(f32)
    # the final pass: the recurrences again, from the carries
    one = f32(1)
    v = xt.copy()
    if mode != ANTICAUSAL:
        prev = c_l
        for i in range(T):
            prev = (one - wt[:, i]) * v[:, i] + wt[:, i] * prev
            v[:, i] = prev
    if mode != CAUSAL:
        acc = d_l
        for i in range(T - 1, -1, -1):
            acc = (one - wt[:, i + 1]) * v[:, i] + wt[:, i + 1] * acc
            v[:, i] = acc
    return v.reshape(-1)[:n]
