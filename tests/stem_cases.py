"""Test helper: the case tables of tests/test_gpu_stem_edges.py, the float64 references of the three stem directions and a restatement of the stem
kernels' BOOKKEEPING in plain Python -- which tile, channel pass, K group, mask word, walk row and template instantiation a case reaches.

The stem (conv 7x7 / stride 2 / pad 3 from the NCHW input) is the one family that skips work based on the data.  What is skipped follows from

    csrc/stem.hip        forward: 4 x 32 output tiles, 13 x 72 input patch (origin hi0 = 2 y0 - 3, patch column p = input column wi0 - 1 + p,
                         wi0 = 2 x0 - 3), NSLOT = 4 resident channels per pass, passes overlapping by one channel, K groups of 8 taps,
                         Kp = ceil(49 C / 8) * 8; the non-zero map [B][C][ceil(H / 4)][ceil(W / 256)], bit (w >> 3) & 31 of a 4 x 8 cell
    csrc/backward.hip    weight gradient: 2 x 32 tiles, 9 x 72 patch, groups of 4 channels (grid.y), Kp = ceil(49 C / 32) * 32, min(ntiles, 256) row
                         blocks walking tile m G + (bx + 97 m) % G of row m, 64 rows per chunk; 14 units of 32 taps per group (u_span)
    csrc/stem_dgrad.hip  data gradient: chunks of 20 channels, stem_dgrad_kernel<5> for the full chunks, <ceil(rest / 4)> for the partial one
    csrc/train.hip       proxy builders: one grid-stride trip covers 64 workgroups x 1024 pixels; float4 stores when wh % 4 == 0

all of which is restated here.  tests/test_stem_cases_cpu.py holds the restated SIZES to the library's exported size functions; the gating rules are
file-local to the kernels: a change of one of them has to be repeated here by hand (the GPU tests then still check the results, and the exact
mask / activity comparisons still check the maps).

Data families:
    dense         det_uniform values: the derived error bounds
    tracer        small integers (x in 0..2, w and dy in -2..2, w varying in all four indices): every result is an integer below 2^24 in any
                  summation order -- a dropped or doubled K group, tap, tile or partial is a wrong integer; compared with ==
    single_pixel  tracer weights, ONE non-zero input pixel, at the positions where the gating changes (derived from the geometry)
    proxy_like    integer blobs in some channels and a silhouette block in channel 0, placed so that the forward tiles see 0, 1, 3, 4, 5, 7, 8 and
                  all channels active
    specials      an all-zero input; cells holding only -0.0 (mask bit 0, same bits as the dense run); one NaN pixel
"""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from detgen import det_uniform

U = 2.0 ** -24

# ------------------------------------------------------------------------------------------------------------------------------------
# geometry

PW = 72
TX = 32
FWD_TY, FWD_PH = 4, 13            # csrc/stem.hip
WG_TY, WG_PH = 2, 9               # csrc/backward.hip
NSLOT = 4
CG = 4
WGRAD_BLOCK_CAP = 256
WGRAD_CHUNK_ROWS = 64
WGRAD_ROT = 97
DG_CCH, DG_NTMAX, DG_KG = 20, 5, 64
DG_TYB, DG_TXB = 4, 32
DGRAD_MAX_CIN = 64
LDS_LIMIT = 160 * 1024


def cdiv(a, b):
    return -(-a // b)


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def tiles(B, H, W, ty):
    """-> (tiles_x, tiles_y, ntiles) of ty x 32 output tiles"""
    Ho, Wo = out_hw(H, W)
    tx_, ty_ = cdiv(Wo, TX), cdiv(Ho, ty)
    return tx_, ty_, B * tx_ * ty_


def patch_rows(tyi, ty, ph, H):
    """input rows of tile row tyi that lie inside the image -> (first, last); hi0 = 2 y0 - 3"""
    hi0 = 2 * tyi * ty - 3
    return max(hi0, 0), min(hi0 + ph - 1, H - 1)


def patch_cols(txi, W):
    """input columns of the 72-column patch of tile column txi inside the image -> (wa, wb); patch column p is input column wi0 - 1 + p"""
    wi0 = 2 * txi * TX - 3
    return max(wi0 - 1, 0), min(wi0 - 2 + PW, W - 1)


def mask_dims(H, W):
    return cdiv(H, 4), cdiv(W, 256)


def stem_weight_floats(C):
    return cdiv(49 * C, 8) * 512


def fwd_kp(C):
    return cdiv(49 * C, 8) * 8


def fwd_lds_bytes(C):
    Kp = fwd_kp(C)
    return (1 + NSLOT) * FWD_PH * PW * 4 + (2 * Kp + C * FWD_PH + 2 * C + 4 * (Kp >> 3)) * 4


def stat_blocks(B, H, W):
    return tiles(B, H, W, FWD_TY)[2]


def nzmask_words(B, C, H, W):
    if B <= 0 or C <= 0 or H <= 0 or W <= 0:
        return 0
    HC, WW = mask_dims(H, W)
    return B * C * HC * WW


def stem_tiles(B, H, W):
    return tiles(B, H, W, WG_TY)[2]


def wgrad_kp(C):
    return cdiv(49 * C, 32) * 32


def wgrad_blocks(ntiles):
    return min(ntiles, WGRAD_BLOCK_CAP)


def wgrad_workspace_layout(B, C, H, W):
    """-> (partial floats, mask words, activity bytes, total bytes): the three regions of the workspace, in this order"""
    nt = stem_tiles(B, H, W)
    part = wgrad_blocks(nt) * 64 * wgrad_kp(C)
    words = nzmask_words(B, C, H, W)
    tact = cdiv(C, CG) * nt
    return part, words, tact, part * 4 + words * 4 + ((tact + 3) & ~3)


def wgrad_workspace_bytes(B, C, H, W):
    return wgrad_workspace_layout(B, C, H, W)[3]


def dgrad_chunks(cin):
    """-> (full chunks, channels of the partial chunk, NT of the partial launch or 0)"""
    full, rest = cin // DG_CCH, cin % DG_CCH
    return full, rest, (rest * 4 + 15) // 16 if rest else 0


def dgrad_weight_floats(cin):
    if cin < 1 or cin > DGRAD_MAX_CIN:
        return 0
    return DG_KG * cdiv(cin, DG_CCH) * DG_NTMAX * 256


# ------------------------------------------------------------------------------------------------------------------------------------
# the non-zero map and what the kernels derive from it

def nzmask_ref(x):
    """x [B][C][H][W] (numpy or torch) -> uint32 words [B][C][HC][WW]: bit (w >> 3) & 31 of word w >> 8 is set when the 4 x 8 cell holds a value
    != 0 (NaN counts, -0.0 does not); columns >= W and rows >= H hold nothing"""
    x = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    B, C, H, W = x.shape
    HC, WW = mask_dims(H, W)
    nz = np.zeros((B, C, HC * 4, WW * 256), bool)
    nz[:, :, :H, :W] = x != 0
    cells = nz.reshape(B, C, HC, 4, WW, 32, 8).any(axis=(3, 6))                       # [B][C][HC][WW][32]
    return (cells.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def mask_cells(mask, B, C, H, W):
    """words -> bool cells [B][C][HC][WW * 32]"""
    HC, WW = mask_dims(H, W)
    m = np.asarray(mask).astype(np.uint32).reshape(B, C, HC, WW, 1)
    return ((m >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(B, C, HC, WW * 32)


def _tile_channels(cells, B, C, H, W, ty, ph):
    """-> bool [B][tiles_y][tiles_x][C]: channel c has a set cell that intersects the tile's patch (rows and columns inside the image)"""
    tx_, ty_, _ = tiles(B, H, W, ty)
    out = np.zeros((B, ty_, tx_, C), bool)
    for tyi in range(ty_):
        r0, r1 = patch_rows(tyi, ty, ph, H)
        for txi in range(tx_):
            wa, wb = patch_cols(txi, W)
            out[:, tyi, txi] = cells[:, :, r0 >> 2:(r1 >> 2) + 1, wa >> 3:(wb >> 3) + 1].any(axis=(2, 3))
    return out


def tile_any_ref(mask, B, C, H, W):
    """straps_stem_tile_activity: uint8 [ntiles] over the weight gradient's 2 x 32 tiles, read from the MASK (the kernels see cells, not pixels)"""
    return _tile_channels(mask_cells(mask, B, C, H, W), B, C, H, W, WG_TY, WG_PH).any(-1).reshape(-1).astype(np.uint8)


def tile_act_ref(mask, B, C, H, W):
    """stem_tileact_kernel: uint8 [groups][ntiles], bit cl = channel 4 grp + cl active in the tile's 9 x 72 patch"""
    act = _tile_channels(mask_cells(mask, B, C, H, W), B, C, H, W, WG_TY, WG_PH).reshape(-1, C)
    groups = cdiv(C, CG)
    out = np.zeros((groups, act.shape[0]), np.uint8)
    for c in range(C):
        out[c // CG] |= (act[:, c].astype(np.uint8) << (c % CG)).astype(np.uint8)
    return out


FwdTile = namedtuple('FwdTile', 'n_active passes list_lengths straddle_boundary straddle_lower straddle_upper')


def fwd_rowflags(cells, b, tyi, txi, C, H, W):
    """the strip flags of stem_kernel for one tile: bool [C][13]"""
    hi0 = 2 * tyi * FWD_TY - 3
    wa, wb = patch_cols(txi, W)
    rf = np.zeros((C, FWD_PH), bool)
    for row in range(FWD_PH):
        hi = hi0 + row
        if 0 <= hi < H:
            rf[:, row] = cells[b, :, hi >> 2, wa >> 3:(wb >> 3) + 1].any(-1)
    return rf


def fwd_tile_reach(rowflag):
    """rowflag bool [C][13] -> FwdTile, plus the per-group contraction count (for the exactly-once property) as a second value"""
    C = rowflag.shape[0]
    K, Kp = 49 * C, fwd_kp(C)
    G = Kp >> 3
    active = rowflag.any(1)
    n_active = int(active.sum())
    rank = np.where(active, np.cumsum(active) - 1, -1)
    k = np.arange(Kp)
    ck, rk = np.minimum(k // 49, C - 1), (k % 49) // 7
    BIG = 1 << 30
    lo = np.empty((4, G), np.int64)
    hi = np.empty((4, G), np.int64)
    flagged = np.empty((4, Kp), bool)
    for wave in range(4):
        fl = (k < K) & rowflag[ck, rk + 2 * wave]
        flagged[wave] = fl
        r = rank[ck]
        lo[wave] = np.where(fl, r, BIG).reshape(G, 8).min(1)
        hi[wave] = np.where(fl, r, -1).reshape(G, 8).max(1)
    counts = np.zeros((4, G), np.int64)
    lengths, passes = set(), 0
    if n_active:
        c0 = 0
        while True:
            nch = min(NSLOT, n_active - c0)
            act = (hi >= 0) & (lo >= c0) & (hi < c0 + nch) & ~((c0 > 0) & (hi == c0))
            counts += act
            lengths |= set(int(v) for v in act.sum(1))
            passes += 1
            if c0 + nch >= n_active:
                break
            c0 += NSLOT - 1
    # straddling groups: the taps of the group belong to two channels (k < K)
    kk = k.reshape(G, 8)
    c_first = kk[:, 0] // 49
    c_last = np.minimum(kk[:, 7], K - 1) // 49
    two = (c_first != c_last) & (kk[:, 0] < K)
    boundary = lower = upper = False
    for wave in range(4):
        fl = flagged[wave].reshape(G, 8)
        isl = (kk // 49) == c_first[:, None]
        has_l, has_u = (fl & isl).any(1), (fl & ~isl & (kk < K)).any(1)
        both = two & has_l & has_u
        boundary = boundary or bool((both & (lo[wave] > 0) & (lo[wave] % (NSLOT - 1) == 0) & (hi[wave] == lo[wave] + 1)).any())
        lower = lower or bool((two & has_l & ~has_u).any())
        upper = upper or bool((two & ~has_l & has_u).any())
    return FwdTile(n_active, passes, frozenset(lengths), boundary, lower, upper), (counts, hi >= 0)


def fwd_reach(mask, shape):
    """mask words (or None: without a map the kernel flags every strip) -> list of FwdTile, one per forward tile in block order"""
    B, C, H, W = shape
    tx_, ty_, _ = tiles(B, H, W, FWD_TY)
    cells = None if mask is None else mask_cells(mask, B, C, H, W)
    out = []
    for b in range(B):
        for tyi in range(ty_):
            for txi in range(tx_):
                rf = np.ones((C, FWD_PH), bool) if cells is None else fwd_rowflags(cells, b, tyi, txi, C, H, W)
                out.append(fwd_tile_reach(rf)[0])
    return out


WgradReach = namedtuple('WgradReach', 'ntiles rows last_partial second_chunk nc_last span_half_active empty_chunk')


def wgrad_units(nc):
    """the channel span (cl0, cl1) of the 7 tap column blocks of a group with nc channels; None for a block behind the group's taps"""
    gk = nc * 49
    return [((32 * nb) // 49, min(32 * nb + 31, gk - 1) // 49) if 32 * nb < gk else None for nb in range(cdiv(CG * 49, 32))]


def wgrad_walk(bx, G, ntiles):
    """the tiles workgroup bx visits, by chunk of 64 walk rows: list of lists"""
    chunks = []
    m0 = 0
    while m0 * G < ntiles:
        ts = [m * G + (bx + WGRAD_ROT * m) % G for m in range(m0, m0 + WGRAD_CHUNK_ROWS)]
        chunks.append([t for t in ts if t < ntiles])
        m0 += WGRAD_CHUNK_ROWS
    return chunks


def wgrad_reach(mask, shape):
    B, C, H, W = shape
    nt = stem_tiles(B, H, W)
    G = wgrad_blocks(nt)
    rows = cdiv(nt, G)
    groups = cdiv(C, CG)
    nc_last = C - CG * (groups - 1)
    tact = tile_act_ref(mask, B, C, H, W)
    half = False
    for grp in range(groups):
        nc = min(CG, C - CG * grp)
        for sp in wgrad_units(nc):
            if sp is not None and sp[0] != sp[1]:
                a, b = (tact[grp] >> sp[0]) & 1, (tact[grp] >> sp[1]) & 1
                half = half or bool((a != b).any())
    empty = False
    if rows > 1:
        for bx in (0, G // 2, G - 1):
            for ch in wgrad_walk(bx, G, nt):
                empty = empty or not any(tact[:, t].any() for t in ch)
    return WgradReach(nt, rows, nt % G != 0, rows > WGRAD_CHUNK_ROWS, nc_last, half, empty)


def proxy_reach(wh):
    """build_proxy_kernel: (vector stores, a second grid-stride trip)"""
    gx = min((wh * wh // 4 + 255) // 256, 64)
    return wh % 4 == 0, wh * wh > gx * 1024


# ------------------------------------------------------------------------------------------------------------------------------------
# packed weights (the layout comments of csrc/stem.hip and csrc/stem_dgrad.hip)

def pack_stem_weight_ref(w):
    """w [64][C][7][7] fp32 -> [G][2][64][4]: element e of lane l of half nt of group g is w[nt * 32 + (l & 31)][8 g + 4 (l >> 5) + e], 0 for k >= 49 C"""
    w = np.asarray(w, np.float32)
    C = w.shape[1]
    K, Kp = 49 * C, fwd_kp(C)
    wk = np.zeros((64, Kp), np.float32)
    wk[:, :K] = w.reshape(64, K)
    g, nt, lane, e = np.meshgrid(np.arange(Kp >> 3), np.arange(2), np.arange(64), np.arange(4), indexing='ij')
    return wk[nt * 32 + (lane & 31), 8 * g + 4 * (lane >> 5) + e].reshape(-1)


def pack_stem_dgrad_weight_ref(w):
    """w [64][C][7][7] -> [KG][nch][5][64][4]: lane = kq * 16 + j, element s: dy channel o = 16 (kg & 3) + 4 kq + s of window tap (d, e) = (kg >> 4,
    (kg >> 2) & 3); column n = nt * 16 + j of chunk ch is channel ch * 20 + (n >> 2), parity (py, px) = ((n >> 1) & 1, n & 1); the value is
    w[o][c][py + 5 - 2 d][px + 5 - 2 e], +0.0 for a tap outside 0..6 and for c >= C"""
    w = np.asarray(w, np.float32)
    C = w.shape[1]
    nch = cdiv(C, DG_CCH)
    kg, ch, nt, lane, s = np.meshgrid(np.arange(DG_KG), np.arange(nch), np.arange(DG_NTMAX), np.arange(64), np.arange(4), indexing='ij')
    tap = kg >> 2
    d, e = tap >> 2, tap & 3
    o = 16 * (kg & 3) + 4 * (lane >> 4) + s
    n = nt * 16 + (lane & 15)
    cl, py, px = n >> 2, (n >> 1) & 1, n & 1
    c = ch * DG_CCH + cl
    r, q = py + 5 - 2 * d, px + 5 - 2 * e
    ok = (c < C) & (r >= 0) & (r < 7) & (q >= 0) & (q < 7)
    v = w[o, np.minimum(c, C - 1), np.clip(r, 0, 6), np.clip(q, 0, 6)]
    return np.where(ok, v, np.float32(0)).astype(np.float32).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------------------------
# float64 references (from the fp32 operands) and their sum_abs

def fwd_reference(x, w):
    """-> (y [B][64][Ho][Wo], sum|x w|) in float64"""
    x, w = x.double(), w.double()
    return F.conv2d(x, w, None, 2, 3), F.conv2d(x.abs(), w.abs(), None, 2, 3)


def wgrad_reference(x, dy):
    """x [B][C][H][W], dy [B][64][Ho][Wo] -> (dw [64][C][7][7], sum|x dy|) in float64"""
    x, dy = x.double(), dy.double()
    shp = (64, x.shape[1], 7, 7)
    return torch.nn.grad.conv2d_weight(x, shp, dy, 2, 3), torch.nn.grad.conv2d_weight(x.abs(), shp, dy.abs(), 2, 3)


def dgrad_reference(dy, w, H, W):
    """dy [B][64][Ho][Wo], w [64][C][7][7] -> (dx [B][C][H][W], sum|dy w|) in float64"""
    dy, w = dy.double(), w.double()
    shp = (dy.shape[0], w.shape[1], H, W)
    return torch.nn.grad.conv2d_input(shp, w, dy, 2, 3), torch.nn.grad.conv2d_input(shp, w.abs(), dy.abs(), 2, 3)


def fwd_loop(x, w):
    """the forward by its definition: explicit loops over (b, o, yo, xo) and a sum over the (c, r, s) window (small cases only)"""
    x, w = x.double().numpy(), w.double().numpy()
    B, C, H, W = x.shape
    Ho, Wo = out_hw(H, W)
    xp = np.zeros((B, C, H + 6, W + 6))
    xp[:, :, 3:3 + H, 3:3 + W] = x
    y = np.zeros((B, 64, Ho, Wo))
    for b in range(B):
        for o in range(64):
            for yo in range(Ho):
                for xo in range(Wo):
                    acc = 0.0
                    for c in range(C):
                        for r in range(7):
                            for s in range(7):
                                acc += xp[b, c, 2 * yo + r, 2 * xo + s] * w[o, c, r, s]
                    y[b, o, yo, xo] = acc
    return torch.from_numpy(y)


def unfold_columns(x):
    """x [B][C][H][W] float64 -> [B][49 C][Ho * Wo]"""
    return F.unfold(x.double(), 7, 1, 3, 2)


def wgrad_unfold(x, dy):
    B = x.shape[0]
    return torch.einsum('bop,bkp->ok', dy.double().reshape(B, 64, -1), unfold_columns(x)).reshape(64, x.shape[1], 7, 7)


def dgrad_fold(dy, w, H, W):
    B, C = dy.shape[0], w.shape[1]
    cols = torch.einsum('ok,bop->bkp', w.double().reshape(64, C * 49), dy.double().reshape(B, 64, -1))
    return F.fold(cols, (H, W), 7, 1, 3, 2)


def window_contains(B, H, W, pix):
    """bool [B][Ho][Wo]: the 7 x 7 window of the output contains input pixel pix = (b, h, w)"""
    Ho, Wo = out_hw(H, W)
    b, h, w = pix
    yo, xo = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    out = np.zeros((B, Ho, Wo), bool)
    out[b] = (2 * yo - 3 <= h) & (h <= 2 * yo + 3) & (2 * xo - 3 <= w) & (w <= 2 * xo + 3)
    return out


def stats_reference(y_nhwc, B, H, W):
    """the per-block statistics partials from the kernel's OWN output y [B][Ho][Wo][64] (fp32): float64 sums over the in-range pixels of every 4 x 32
    tile -> (sum [nblk][64], sumsq, sum|y|, n in-range pixels [nblk]); block index = (b * tiles_y + ty) * tiles_x + tx"""
    Ho, Wo = out_hw(H, W)
    tx_, ty_, nblk = tiles(B, H, W, FWD_TY)
    yp = torch.zeros(B, ty_ * FWD_TY, tx_ * TX, 64, dtype=torch.float64)
    yp[:, :Ho, :Wo] = y_nhwc.double()
    t = yp.view(B, ty_, FWD_TY, tx_, TX, 64)
    one = torch.zeros(B, ty_ * FWD_TY, tx_ * TX, dtype=torch.float64)
    one[:, :Ho, :Wo] = 1
    n = one.view(B, ty_, FWD_TY, tx_, TX).sum((2, 4)).reshape(nblk)
    return t.sum((2, 4)).reshape(nblk, 64), (t * t).sum((2, 4)).reshape(nblk, 64), t.abs().sum((2, 4)).reshape(nblk, 64), n


# ------------------------------------------------------------------------------------------------------------------------------------
# data

FWD_SHAPES = [(1, 1, 7, 7), (3, 2, 9, 13), (2, 3, 8, 66), (1, 4, 16, 128), (1, 5, 10, 68), (1, 7, 12, 72), (1, 8, 8, 64), (2, 18, 33, 50), (1, 64, 7, 7),
              (1, 18, 12, 264), (1, 6, 8, 516), (1, 18, 12, 261)]
WGRAD_BIG = [(7, 5, 64, 136), (8193, 2, 7, 7)]
WGRAD_SHAPES = FWD_SHAPES + WGRAD_BIG
SINGLE_SHAPES = [(1, 2, 9, 13), (1, 3, 8, 66), (1, 18, 33, 50), (1, 6, 8, 516), (1, 18, 12, 261)]      # (B = 1: one pixel in the whole tensor)
PROXY_SHAPES = [(1, 18, 12, 264), (1, 18, 12, 261), (2, 18, 33, 50), (1, 7, 12, 72), (7, 5, 64, 136)]
SPECIAL_SHAPES = [(3, 2, 9, 13), (1, 18, 12, 264)]
FUSED_SHAPES = [(3, 2, 9, 13), (1, 4, 16, 128), (1, 18, 12, 264)]                                      # one ragged, one full, one W > 256
DETERMINISM_SHAPE = (2, 18, 33, 50)

DGRAD_CIN = (5, 9, 13, 20, 25, 29, 33, 40)
DGRAD_HW = ((9, 13), (8, 66))
DGRAD_B = (1, 3)

PROXY_STD_WH = (18, 21, 24, 40, 64, 264)
PROXY_NZ_WH = (24, 40, 64, 264)


def proxy_stds(wh):
    return sorted({1, 2, wh // 4})


def idx4(shape):
    return np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')


def tracer_w(C):
    o, c, r, s = idx4((64, C, 7, 7))
    return torch.from_numpy((((3 * o + 5 * c + 7 * r + s) % 5) - 2).astype(np.float32))


def tracer_x(shape):
    b, c, h, w = idx4(shape)
    return torch.from_numpy(((7 * b + 3 * c + 5 * h + w + (h * w) % 4) % 3).astype(np.float32))


def tracer_dy(B, Ho, Wo):
    """NCHW [B][64][Ho][Wo], integers -2..2"""
    b, o, y, x = idx4((B, 64, Ho, Wo))
    return torch.from_numpy((((3 * b + 5 * o + 7 * y + x) % 5) - 2).astype(np.float32))


_PERIOD = (1 << 19) + 17


def det(shape, seed, lo=-1.0, hi=1.0):
    """det_uniform as a CPU tensor; beyond 2^19 elements one block repeated (an odd period against every extent of the tables)"""
    n = int(np.prod(shape))
    if n <= _PERIOD:
        return torch.from_numpy(det_uniform(tuple(shape), seed, lo, hi))
    blk = torch.from_numpy(det_uniform((_PERIOD,), seed, lo, hi))
    return blk.repeat(cdiv(n, _PERIOD))[:n].view(tuple(shape)).contiguous()


def dense_w(C, seed=7):
    return det((64, C, 7, 7), seed) * float((2.0 / (C * 49)) ** 0.5)


def body_keep(B):
    """the large weight-gradient case: most bodies all zero; the last body (the tiles of the second 64-row chunk) is kept"""
    b = np.arange(B)
    return torch.from_numpy((b % 97 == 0) | (b == B - 1))


def single_pixel_positions(shape):
    """(c, h, w) of the one non-zero pixel, derived from the geometry: where a tile's patch, a cell or a mask word begins or ends"""
    B, C, H, W = shape
    wi0_1 = 2 * TX - 3                                     # tile column 1 of either direction
    cols = {0, W - 1, wi0_1 - 1, wi0_1, -3 + 68, -3 + 69, -3 + 70, 7, 8, 255, 256}
    rows = {0, H - 1, 3, 4}
    for ty, ph in ((FWD_TY, FWD_PH), (WG_TY, WG_PH)):      # first and last patch row of tile row 1
        rows |= {2 * ty - 3, 2 * ty - 3 + ph - 1}
    cols = sorted(c for c in cols if 0 <= c < W)
    rows = sorted(r for r in rows if 0 <= r < H)
    mid_r, mid_c = rows[len(rows) // 2], cols[len(cols) // 2]
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + [(mid_r, c) for c in cols] + [(r, mid_c) for r in rows]
    out, seen = [], set()
    for i, (h, w) in enumerate(pos):
        if (h, w) not in seen:
            seen.add((h, w))
            out.append(((3 * i + 1) % C, h, w))
    return out


def single_pixel_x(shape, pos):
    x = torch.zeros(shape)
    c, h, w = pos
    x[0, c, h, w] = 2.0 if (h + w) % 2 else 1.0
    return x


# proxy_like: per forward tile (4 x 32 outputs, 64 input columns), `n` channels get a blob inside columns that only this tile column reads; `both`
# of them in a row cell that two tile rows read, the others in a row cell that only the upper one reads
def proxy_like_x(shape):
    B, C, H, W = shape
    x = torch.zeros(shape)
    tx_, ty_, _ = tiles(B, H, W, FWD_TY)
    # (channels with a blob in rows 8 band .. + 3, channels with a blob in rows 8 band + 4 .. + 7): the first i < n of one channel sequence each.  At
    # H <= 12 there are two tile rows and one band: row cell 0 is read by tile row 0 alone, row cell 1 by both -- tile (0, t) sees max(up, shared)
    # channels, tile (1, t) sees `shared`: 1 | 0, 4 | 3, 7 | 5, C | 8, and nothing in the last, narrow tile column
    plans = [(1, 0), (4, 3), (7, 5), (C, 8), (0, 0), (0, 1), (3, 4), (0, 7)]
    for b in range(B):
        for txi in range(tx_):
            for band in range(0, 1 if H <= 12 else cdiv(H, 8)):
                up, shared = plans[(3 * b + txi + 2 * band) % len(plans)]
                up, shared = min(up, C), min(shared, C)
                c_lo = 64 * txi + 8                                                             # cells [64 t + 8, 64 t + 56): inside tile column t alone
                if c_lo + 8 > W:
                    continue
                for i in range(max(up, shared)):
                    c = (5 * i + 2 * txi + b + band) % C if C % 5 else (3 * i + txi + b + band) % C
                    col = c_lo + 8 * (i % 5)
                    if col + 8 > min(W, 64 * txi + 56):
                        col = c_lo
                    for (cnt, r0) in ((up, 8 * band), (shared, 8 * band + 4)):
                        if i < cnt and r0 < H:
                            hh, ww = min(4, H - r0), min(16, W - col)
                            r, q = np.meshgrid(np.arange(hh), np.arange(ww), indexing='ij')
                            x[b, c, r0:r0 + hh, col:col + ww] = torch.from_numpy((1 + (r + q + c) % 2).astype(np.float32))
    if H >= 16 and W >= 100:
        x[:, 0, H // 4:3 * H // 4, 40:90] = 1.0                                                # silhouette-like block
    elif W >= 256:
        x[:, 0, 0:4, 64 * 3 + 8:64 * 3 + 56] = 1.0                                             # (inside the tile that has every channel active)
    return x


def special_x(shape, kind):
    B, C, H, W = shape
    if kind == 'zero':
        return torch.zeros(shape)
    x = det(shape, 60, 0.1, 1.0)
    if kind == 'negzero':                                   # every other cell column, and a whole row band, hold only -0.0
        w = torch.arange(W)
        x[:, :, :, ((w >> 3) % 2) == 1] = -0.0
        x[:, :, 4:8] = -0.0
        return x
    assert kind == 'nan'
    x = x * (torch.arange(W) % 16 < 8)                      # some zero cells as well
    b, c, h, w = nan_pixel(shape)
    x[b, c, h, w] = float('nan')
    return x


def nan_pixel(shape):
    B, C, H, W = shape
    return B - 1, C - 1, H // 2, min(W - 1, 61)


Case = namedtuple('Case', 'id family shape arg')


def sid(shape):
    return 'x'.join(str(s) for s in shape)


def cases(direction):
    """direction 'fwd' | 'wgrad' -> list of Case"""
    out = []
    shapes = FWD_SHAPES if direction == 'fwd' else WGRAD_SHAPES
    for s in shapes:
        out.append(Case('dense-' + sid(s), 'dense', s, None))
        out.append(Case('tracer-' + sid(s), 'tracer', s, None))
    for s in SINGLE_SHAPES:
        for p in single_pixel_positions(s):
            out.append(Case('single-%s-c%dh%dw%d' % ((sid(s),) + p), 'single_pixel', s, p))
    for s in PROXY_SHAPES:
        if direction == 'wgrad' or s in FWD_SHAPES or s[0] == 1:
            out.append(Case('proxy-' + sid(s), 'proxy_like', s, None))
    for s in SPECIAL_SHAPES:
        for kind in ('zero', 'negzero', 'nan'):
            out.append(Case('%s-%s' % (kind, sid(s)), 'specials', s, kind))
    return out


def case_x(case):
    s = case.shape
    if case.family == 'dense':
        x = det(s, 6, 0.0, 1.0)
        return x * body_keep(s[0])[:, None, None, None] if s[0] > 1000 else x
    if case.family == 'tracer':
        x = tracer_x(s)
        return x * body_keep(s[0])[:, None, None, None] if s[0] > 1000 else x
    if case.family == 'single_pixel':
        return single_pixel_x(s, case.arg)
    if case.family == 'proxy_like':
        return proxy_like_x(s)
    return special_x(s, case.arg)


def case_integer(case):
    return case.family in ('tracer', 'single_pixel', 'proxy_like')


def case_w(case):
    return tracer_w(case.shape[1]) if case_integer(case) else dense_w(case.shape[1])


def case_dy(case):
    B, C, H, W = case.shape
    Ho, Wo = out_hw(H, W)
    return tracer_dy(B, Ho, Wo) if case_integer(case) else det((B, 64, Ho, Wo), 8)


@functools.lru_cache(maxsize=None)
def case_mask(case):
    return nzmask_ref(case_x(case))


def dgrad_cases():
    """(cin, B, H, W): every channel count of the forward shapes, and the counts that select the instantiations no test had launched"""
    out = [(c, b, h, w) for c in DGRAD_CIN for (h, w) in DGRAD_HW for b in DGRAD_B]
    out += [(C, B, H, W) for (B, C, H, W) in FWD_SHAPES]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# reach table

REQUIRED = [
    ('stem_nzmask_kernel', 'vector'), ('stem_nzmask_kernel', 'scalar'), ('stem_nzmask_kernel', 'partial last cell rows'),
    ('stem_nzmask_kernel', 'partial last cell columns'),
    ('stem_kernel', 'vector fill'), ('stem_kernel', 'scalar fill'),
    ('mask row', '1 word'), ('mask row', '2 words'), ('mask row', '3 words'), ('mask row', 'patch straddles 255|256'), ('mask row', 'b1 == 31 inside the image'),
    ('stem_kernel', 'n_active 0'), ('stem_kernel', 'n_active 1'), ('stem_kernel', 'n_active 4'), ('stem_kernel', 'n_active 5'), ('stem_kernel', 'n_active 7'),
    ('stem_kernel', 'n_active 8'), ('stem_kernel', 'n_active C'), ('stem_kernel', 'n_active 3'), ('stem_kernel', '0 < n_active < C'),
    ('stem_kernel', 'passes 1'), ('stem_kernel', 'passes 2'), ('stem_kernel', 'passes 3'), ('stem_kernel', 'passes 6'),
    ('stem_kernel', 'list length 0'), ('stem_kernel', 'list length 1'), ('stem_kernel', 'list length 2'),
    ('stem_kernel', 'straddle across ranks 3|4'), ('stem_kernel', 'straddle across ranks 6|7'),
    ('stem_kernel', 'straddle lower only'), ('stem_kernel', 'straddle upper only'),
    ('stem_kernel', 'K padding'), ('stem_kernel', 'no K padding'), ('stem_kernel', 'ragged tile'), ('stem_kernel', 'full tile'),
    ('stem_dgrad_kernel', '<1>'), ('stem_dgrad_kernel', '<2>'), ('stem_dgrad_kernel', '<3>'), ('stem_dgrad_kernel', '<4>'), ('stem_dgrad_kernel', '<5> partial'),
    ('stem_dgrad_kernel', '<1> after full'), ('stem_dgrad_kernel', '<2> after full'), ('stem_dgrad_kernel', '<3> after full'),
    ('stem_dgrad_kernel', '<4> after full'), ('stem_dgrad_kernel', 'full only'), ('stem_dgrad_kernel', 'two full chunks'),
    ('stem_wgrad_kernel', 'rows 1'), ('stem_wgrad_kernel', 'rows > 1, last partial'), ('stem_wgrad_kernel', 'second chunk'),
    ('stem_wgrad_kernel', 'empty chunk'), ('stem_wgrad_kernel', 'nc 1'), ('stem_wgrad_kernel', 'nc 2'), ('stem_wgrad_kernel', 'nc 3'),
    ('stem_wgrad_kernel', 'nc 4'), ('stem_wgrad_kernel', 'span half active'), ('stem_wgrad_kernel', 'vector fill'), ('stem_wgrad_kernel', 'scalar fill'),
    ('build_proxy_kernel', 'vector, 1 trip'), ('build_proxy_kernel', 'scalar, 1 trip'), ('build_proxy_kernel', 'vector, 2 trips'),
    ('build_proxy_nz_kernel', '1 word'), ('build_proxy_nz_kernel', '2 words'),
]

UNREACHABLE = {
    ('stem_kernel', 'a pass with n_active == 0'): 'the channel passes run only when some strip of the tile is flagged (tile_any), and a flagged strip makes its channel '
                                                  'active: an all-zero tile goes straight to the epilogue',
    ('stem_kernel', 'a K group over three channels'): 'a group is 8 consecutive taps and a channel has 49: a group touches at most two channels, whatever C',
    ('stem_wgrad_kernel', 'a unit over three channels'): 'a unit is 32 consecutive taps of a group and a channel has 49',
    ('build_proxy_kernel', 'scalar, 2 trips'): 'a second trip needs wh * wh > 65536 with wh % 4 != 0, the smallest being wh = 257: a 66 049-pixel plane per channel and an '
                                               'oracle loop of that size for a store form the one-trip case already runs; the trip count does not depend on the store form',
}


def _mask_row_reach(shape, direction):
    B, C, H, W = shape
    got = {('mask row', '%d word%s' % (mask_dims(H, W)[1], '' if mask_dims(H, W)[1] == 1 else 's'))}
    ty = FWD_TY if direction == 'fwd' else WG_TY
    for txi in range(tiles(B, H, W, ty)[0]):
        wa, wb = patch_cols(txi, W)
        if wa >> 8 != wb >> 8:
            got.add(('mask row', 'patch straddles 255|256'))
        for word in range(wa >> 8, (wb >> 8) + 1):
            hi_c = min(wb, (word << 8) + 255)
            if (hi_c >> 3) & 31 == 31 and hi_c < W - 1:
                got.add(('mask row', 'b1 == 31 inside the image'))
    return got


def reached():
    """-> {(kernel, branch): [case ids]}"""
    got = {}

    def add(key, cid):
        ids = got.setdefault(key, [])
        if not ids or ids[-1] != cid:
            ids.append(cid)

    for case in cases('fwd'):
        B, C, H, W = case.shape
        Ho, Wo = out_hw(H, W)
        add(('stem_nzmask_kernel', 'vector' if W % 4 == 0 else 'scalar'), case.id)
        add(('stem_kernel', 'vector fill' if W % 4 == 0 else 'scalar fill'), case.id)
        if H % 4:
            add(('stem_nzmask_kernel', 'partial last cell rows'), case.id)
        if W % 8:
            add(('stem_nzmask_kernel', 'partial last cell columns'), case.id)
        for k in _mask_row_reach(case.shape, 'fwd'):
            add(k, case.id)
        add(('stem_kernel', 'K padding' if 49 * C % 8 else 'no K padding'), case.id)
        if Ho % FWD_TY or Wo % TX:
            add(('stem_kernel', 'ragged tile'), case.id)
        if Ho >= FWD_TY and Wo >= TX:
            add(('stem_kernel', 'full tile'), case.id)
        for t in fwd_reach(case_mask(case), case.shape):
            n = t.n_active
            for v in (0, 1, 3, 4, 5, 7, 8):
                if n == v:
                    add(('stem_kernel', 'n_active %d' % v), case.id)
            if n == C:
                add(('stem_kernel', 'n_active C'), case.id)
            if 0 < n < C:
                add(('stem_kernel', '0 < n_active < C'), case.id)
            if t.passes in (1, 2, 3, 6):
                add(('stem_kernel', 'passes %d' % t.passes), case.id)
            for L in (0, 1, 2):
                if L in t.list_lengths:
                    add(('stem_kernel', 'list length %d' % L), case.id)
            if t.straddle_lower:
                add(('stem_kernel', 'straddle lower only'), case.id)
            if t.straddle_upper:
                add(('stem_kernel', 'straddle upper only'), case.id)
        for t in fwd_reach(case_mask(case), case.shape):
            if t.straddle_boundary:
                if t.n_active >= 5:
                    add(('stem_kernel', 'straddle across ranks 3|4'), case.id)
                if t.n_active >= 8:
                    add(('stem_kernel', 'straddle across ranks 6|7'), case.id)
    for case in cases('wgrad'):
        B, C, H, W = case.shape
        r = wgrad_reach(case_mask(case), case.shape)
        add(('stem_wgrad_kernel', 'vector fill' if W % 4 == 0 else 'scalar fill'), case.id)
        add(('stem_wgrad_kernel', 'rows 1') if r.rows == 1 else ('stem_wgrad_kernel', 'rows > 1, last partial') if r.last_partial else ('stem_wgrad_kernel', 'rows > 1'), case.id)
        if r.second_chunk:
            add(('stem_wgrad_kernel', 'second chunk'), case.id)
        if r.empty_chunk:
            add(('stem_wgrad_kernel', 'empty chunk'), case.id)
        add(('stem_wgrad_kernel', 'nc %d' % r.nc_last), case.id)
        if r.span_half_active:
            add(('stem_wgrad_kernel', 'span half active'), case.id)
        for k in _mask_row_reach(case.shape, 'wgrad'):
            add(k, case.id)
    for (cin, B, H, W) in dgrad_cases():
        full, rest, nt = dgrad_chunks(cin)
        cid = 'dgrad-cin%d-%dx%dx%d' % (cin, B, H, W)
        if rest == 0:
            add(('stem_dgrad_kernel', 'full only'), cid)
        elif nt == 5:
            add(('stem_dgrad_kernel', '<5> partial'), cid)
        else:
            add(('stem_dgrad_kernel', '<%d>%s' % (nt, ' after full' if full else '')), cid)
        if full == 2:
            add(('stem_dgrad_kernel', 'two full chunks'), cid)
    for wh in PROXY_STD_WH:
        vec, two = proxy_reach(wh)
        add(('build_proxy_kernel', '%s, %d trip%s' % ('vector' if vec else 'scalar', 2 if two else 1, 's' if two else '')), 'proxy-std-%d' % wh)
    for wh in PROXY_NZ_WH:
        add(('build_proxy_nz_kernel', '%d word%s' % (cdiv(wh, 256), 's' if wh > 256 else '')), 'proxy-nz-%d' % wh)
    return got
