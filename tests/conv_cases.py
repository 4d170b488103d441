"""Test helper: the case tables of tests/test_gpu_conv_edges.py and a statement of WHICH KERNEL each case reaches.

The convolution family picks its kernel instantiation from the geometry by size rules, which live in two plans: csrc/conv_plan.h (forward and data
gradient: conv.hip, conv_x3.hip, conv_x3_lean.hip, conv_x3f.hip, conv_bf16.hip launch from it) and csrc/conv_wgrad_plan.h (weight gradients: conv_wgrad.hip,
conv_wgrad_x3f.hip).  This module restates those rules in Python -- limited to what the tables need -- so that every case can say which instantiation
and which epilogue form the library runs for it:

    pick_tile_x3 / halo_patch_slots / halo_choice / lean_epilogue_choice / x3_route        the plane kernels (conv_plan.h: conv_plan_x3)
    pick_tile_x3f / stream_bn / stream_workgroups / x3f_route                              the fp32-operand 1x1 route (conv_plan_x3f)
    x3_lds_bytes / x3f_lds_bytes / bf16_lds_bytes / launch_grid                            dynamic LDS and grid of an instantiation
    wgrad3_plan / wgrad_x3_route / wgrad_x3_block / wgrad_plan                             weight gradients on planes and on fp32 tensors
    wgrad_x3f_block / wgrad_x3f_plan                                                       weight gradient of the fp32-operand route
    pick_tile_bf16 / bf16_refusal / bf16_route / bf16_nchunks                              the single-product bf16 inference route (conv_bf16.hip;
                                                                                           the cases of tests/test_gpu_conv_bf16_edges.py)

tests/test_conv_cases_cpu.py holds the restatement to the plans the built library shows without a launch (straps_conv_plan, straps_conv_wgrad_plan:
instantiation, row tile, partial blocks, grid, LDS; and the block-count, workspace and route queries that wrap them) for every case, and asserts that the tables together reach every instantiation the product library can dispatch to (REQUIRED below; the
ones no network layer reaches are in UNREACHABLE with the reason).  A later change of a size rule that moves a case off its kernel fails there.

An instantiation is named by a tuple:
    ('x3', cfg, epi)            conv_igemm_x3_kernel of tile configuration cfg (1-5, 7-12), epi 0 = shared epilogue, 1 / 2 = the lean forms
    ('x3h', halo, epi)          conv_igemm_x3h_kernel: halo 1 = 128x128 two patch buffers, 2 = 128x64 two buffers, 3 = 128x64 one buffer
    ('x3f', cfg, epi, abn)      conv_igemm_x3f_kernel of tile 1 (128x64) / 2 (64x64); abn: BatchNorm in the operand path
    ('x3f_stream', bn, epi, abn) conv1x1_stream_kernel, 256 (resident weights) / 128 / 64 wide
    ('wgrad3_x3', cp)           conv_wgrad3x3_x3_kernel with 32- or 64-pixel chunks;  ('wgrad3_f32',) conv_wgrad3x3_kernel
    ('wgrad_x3', bco, bci)      conv_wgrad_x3_kernel;  ('wgrad_f32', b) conv_wgrad_kernel<b, b>;  ('wgrad_x3f', bco, bci, abn) conv_wgrad_x3f_kernel
    ('bf16', cfg)               tile configuration cfg (1-10) of conv_bf16.hip: conv_igemm_x3_kernel / conv_igemm_x3h_kernel with PL chunks per stage, EPI = 3
"""
from collections import namedtuple

# ------------------------------------------------------------------------------------------------------------------------------------
# problem geometry (conv_igemm.h: conv_fwd_problem / conv_dgrad_problem)

Cls = namedtuple('Cls', 'Mh Mw M oah oaw ntaps taps')          # taps: ((dh, dw), ...)
Prob = namedtuple('Prob', 'kind B H W Cin Cout stride OH OW omul cls')      # H, W, Cin: the GEMM's source tensor; Cout: its columns


def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def fwd_problem(B, H, W, cin, cout, k, stride, pad):
    mh, mw = out_hw(H, W, k, stride, pad)
    taps = tuple((r - pad, s - pad) for r in range(k) for s in range(k))
    return Prob('fwd', B, H, W, cin, cout, stride, mh, mw, 1, (Cls(mh, mw, B * mh * mw, 0, 0, k * k, taps),))


def dgrad_problem(B, H, W, cin, cout, k, stride, pad):
    """data gradient of a cin -> cout convolution over a [B][H][W][cin] input: a GEMM over dy [B][ho][wo][cout] with cin columns, one class per
    output parity at stride 2 (classes without pixels are dropped; classes without taps -- the dead positions of a 1x1 filter -- stay), heaviest
    class first (stable)."""
    ho, wo = out_hw(H, W, k, stride, pad)
    padh = k - 1 - pad
    cls = []
    for ph in range(stride):
        for pw in range(stride):
            mh, mw = (H - ph + stride - 1) // stride, (W - pw + stride - 1) // stride
            if mh <= 0 or mw <= 0:
                continue
            taps = []
            for r in range(k):
                nh = ph - padh + r
                if nh % stride:
                    continue
                for s in range(k):
                    nw = pw - padh + s
                    if nw % stride:
                        continue
                    taps.append((nh // stride if nh >= 0 else -((-nh) // stride), nw // stride if nw >= 0 else -((-nw) // stride)))
            cls.append(Cls(mh, mw, B * mh * mw, ph, pw, len(taps), tuple(taps)))
    for a in range(1, len(cls)):          # the library's insertion sort: strictly heavier moves forward
        b = a
        while b > 0 and cls[b].ntaps * cls[b].M > cls[b - 1].ntaps * cls[b - 1].M:
            cls[b], cls[b - 1] = cls[b - 1], cls[b]
            b -= 1
    return Prob('dgrad', B, ho, wo, cout, cin, 1, H, W, stride, tuple(cls))


# ------------------------------------------------------------------------------------------------------------------------------------
# the plane kernels (conv_x3.hip)

X3_BM = {1: 128, 2: 128, 3: 64, 4: 256, 5: 128, 7: 128, 8: 128, 9: 128, 10: 128, 11: 128, 12: 256}
X3_BN = {1: 128, 2: 64, 3: 64, 4: 128, 5: 128, 7: 64, 8: 128, 9: 128, 10: 64, 11: 64, 12: 128}
X3_TILES = tuple(sorted(X3_BM))
LEAN_TILES = (3, 5, 7, 9, 11, 12)
# tile_cfg bits: 256 = im2col kernel only, 512 = halo kernel wherever it applies, 1024 = with 512: the single-buffer halo kernel.  Bits 64 / 128 select
# ablation instantiations in the tools build only; the product library ignores them except that a launch with either takes the shared epilogue -- the
# way to reach a halo kernel's shared-epilogue form with a training step's operands (the halo kernels have no tile number to name).  PRODUCT library
# only: in a tools build the bit selects an ablation kernel that is wrong by design (the GPU file asserts which library is loaded).
SHARED_EPILOGUE_BIT = 64


def pick_tile_x3(cfg, M, cout, ncls=1, one_tap=False):
    """-> (cfg, bm, bn) of conv_x3.hip's pick_tile_x3 (product build: no A/B switches)"""
    cfg &= 15
    if cfg == 6:
        cfg = 4
    if cfg == 0:
        t128 = ((M + 127) // 128) * (cout // 128)
        if cout % 128 != 0:
            cfg = 11
        elif t128 // ncls < 128:
            cfg = 3
        elif ncls > 1:
            cfg = 12 if t128 // ncls >= 512 else ((9 if one_tap else 12) if t128 // ncls >= 256 else 11)
        else:
            cfg = 12 if t128 >= 512 else 5 if t128 >= 256 else 7
    if cout % 128 != 0 and cfg not in (3, 7, 10, 11):
        cfg = 2
    bm = 256 if cfg in (4, 6, 12) else 64 if cfg == 3 else 128
    bn = 64 if cfg in (2, 3, 7, 10, 11) else 128
    return cfg, bm, bn


def halo_patch_slots(p):
    BM = 128
    if len(p.cls) != 1 or p.stride != 1 or p.omul != 1:
        return 0
    c = p.cls[0]
    if c.ntaps != 9 or c.Mh != p.H or c.Mw != p.W or p.OH != p.H or p.OW != p.W or c.oah or c.oaw or c.M % BM:
        return 0
    if any(not (-1 <= dh <= 1 and -1 <= dw <= 1) for dh, dw in c.taps):
        return 0
    HW = p.H * p.W
    if BM >= HW:
        return 0 if BM % HW else (BM // HW) * (p.H + 2) * (p.W + 2)
    if BM % p.W or HW % BM:
        return 0
    return (BM // p.W + 2) * (p.W + 2)


def halo_choice(p, tile_cfg):
    if (tile_cfg & 15) != 0 or (tile_cfg & 256):
        return 0
    slots = halo_patch_slots(p)
    all_ = bool(tile_cfg & 512)
    t128 = (p.cls[0].M // 128) * (p.Cout // 128)
    if slots > 0 and p.Cout % 128 != 0 and slots <= 272 and (not all_ or (tile_cfg & 1024)):
        return 3
    if slots > 0 and p.Cout % 128 == 0 and slots <= 208 and (all_ or 256 <= t128 < 512):
        return 1
    if slots > 0 and p.Cout % 128 != 0 and slots <= 272 and all_:
        return 2
    return 0


def lean_epilogue_choice(p, ops):
    """conv_igemm.h.  ops: the operands of the launch, a set of 'y', 'stats', 'scale', 'relu', 'res' (residual / addend), 'res_bits', 'bnr_raw' (fused
    BatchNorm sums), 'bnr_out' (their mask as an fp32 tensor), 'yplanes'.  -> 1 lean forward form, 2 lean data-gradient form, 0 shared epilogue"""
    if 'yplanes' in ops or 'bnr_out' in ops or 'y' not in ops or 'scale' in ops or 'relu' in ops:
        return 0
    c = p.cls[0]
    remap = p.omul != 1 or c.oah != 0 or c.oaw != 0 or p.OH != c.Mh or p.OW != c.Mw
    if 'res' not in ops and 'bnr_raw' not in ops and 'res_bits' not in ops:
        return 1 if (len(p.cls) == 1 and not remap) else 0
    if 'stats' not in ops and ('res' in ops or 'bnr_raw' in ops) and ('res_bits' not in ops or 'res' in ops):
        return 0 if any(c.ntaps == 0 for c in p.cls) else 2
    return 0


def _m_kdim(p):
    return sum(c.M for c in p.cls), max(c.ntaps * p.Cin for c in p.cls)


def x3_route(p, tile_cfg, ops):
    """-> (instantiation, bm, blocks): which kernel dispatch_x3 launches, its row tile and the number of M tiles over all classes"""
    halo = halo_choice(p, tile_cfg)
    M, kdim = _m_kdim(p)
    one_tap = kdim == p.Cin
    cfg, bm, bn = pick_tile_x3(tile_cfg, M, p.Cout, len(p.cls), one_tap)
    blocks = p.cls[0].M // 128 if halo else sum(-(-c.M // bm) for c in p.cls)
    if halo:
        bm = 128
    if (tile_cfg & 15) == 0 and not (tile_cfg & (64 | 128)):
        epi = lean_epilogue_choice(p, ops)
        if epi and (halo in (1, 3) or (not halo and cfg in LEAN_TILES)):
            return (('x3h', halo, epi) if halo else ('x3', cfg, epi)), bm, blocks
    if halo:
        return ('x3h', halo, 0), bm, blocks
    return ('x3', cfg if cfg in X3_BM else 7, 0), bm, blocks


def x3_stat_blocks(B, H, W, cin, cout, k, stride, pad, tile_cfg):
    """straps_conv_x3_stat_blocks"""
    return x3_route(fwd_problem(B, H, W, cin, cout, k, stride, pad), tile_cfg, {'y', 'stats'})[2]


def dgrad_x3_bn_blocks(B, H, W, cin, cout, k, stride, pad, tile_cfg):
    """straps_conv_dgrad_x3_bn_blocks"""
    return x3_route(dgrad_problem(B, H, W, cin, cout, k, stride, pad), tile_cfg, {'y', 'res', 'bnr_raw'})[2]


# (wave rows, wave columns, ring stages) of the plane tiles and (.., patch slots, patch buffers) of the halo forms: conv_plan.h kX3Tile / kX3Halo
X3_WAVES_STAGES = {1: (4, 2, 3), 2: (2, 2, 2), 3: (2, 2, 3), 4: (4, 2, 2), 5: (2, 2, 3), 7: (2, 2, 3), 8: (2, 2, 3), 9: (4, 2, 3), 10: (2, 2, 3), 11: (2, 2, 2), 12: (4, 2, 2)}
X3_HALO_FORMS = {1: (128, 2, 2, 3, 208, 2), 2: (64, 2, 2, 3, 272, 2), 3: (64, 2, 2, 2, 272, 1)}      # bn first


def x3_lds_bytes(inst):
    """dynamic LDS and threads of a plane instantiation: stages x three planes x (BM + BN) rows of 32 bf16; the halo forms hold patch buffers of `slots`
    pixels in the A rows' place"""
    if inst[0] == 'x3h':
        bn, wm, wn, nst, slots, pbuf = X3_HALO_FORMS[inst[1]]
        return (pbuf * 3 * slots + nst * 3 * bn) * 32 * 2, 64 * wm * wn
    wm, wn, nst = X3_WAVES_STAGES[inst[1]]
    return nst * 3 * (X3_BM[inst[1]] + X3_BN[inst[1]]) * 32 * 2, 64 * wm * wn


def launch_grid(p, bm, bn):
    """(grid x, grid y) of the tile kernels: one grid row per class, as wide as the largest class"""
    return max(-(-c.M // bm) for c in p.cls) * (p.Cout // bn), len(p.cls)


# ------------------------------------------------------------------------------------------------------------------------------------
# the fp32-operand 1x1 route (conv_x3f.hip)

def x3f_supported(cin, cout, k, stride, pad):
    return int(k == 1 and pad == 0 and stride in (1, 2) and cin % 64 == 0 and cout % 64 == 0)


def x3f_epilogue(p, ops):
    return 0 if p.cls[0].ntaps != 1 else lean_epilogue_choice(p, ops)


def stream_bn(p, ops):
    if len(p.cls) != 1 or p.cls[0].ntaps != 1 or p.Cin % 64 != 0 or x3f_epilogue(p, ops) == 0:
        return 0
    if p.Cout % 256 == 0 and p.Cin <= 64:
        return 256
    return 128 if (p.Cout % 128 == 0 and p.Cin < p.Cout) else 64


def pick_tile_x3f(cfg, M, cout, ncls, sbn=0):
    """-> (cfg, bm, bn)"""
    cfg &= 15
    if (cfg == 5 or (cfg == 0 and M >= 4 * 128 * (256 // (cout // (sbn if sbn else cout))))) and sbn:
        return 5, (64 if sbn == 256 else 128), sbn
    if cfg == 5:
        cfg = 0
    if cfg == 0:
        t64 = ((M // ncls + 127) // 128) * (cout // 64)
        cfg = 2 if t64 < 512 else 1
    if cfg < 1 or cfg > 2:
        cfg = 1
    return cfg, (64 if cfg == 2 else 128), 64


def stream_lds_bytes(bm, bn, wgm, bres, cin):
    return 2 * 3 * bm * 32 * 2 + 3 * (cin // 32 if bres else 2) * bn * 32 * 2 + wgm * bn * 4 * 4 + 2 * cin * 4


def stream_workgroups(p, bn):
    """(workgroups per N tile of the persistent streaming kernel, its M tiles)"""
    bm = 64 if bn == 256 else 128
    lds = stream_lds_bytes(bm, bn, 2, bn == 256, p.Cin)
    assert lds <= 160 * 1024
    per_cu = min(2, (160 * 1024) // lds)
    mt = -(-p.cls[0].M // bm)
    return max(1, min(256 * per_cu // (p.Cout // bn), mt)), mt


def x3f_route(p, tile_cfg, ops):
    """-> (instantiation, bm, blocks).  ops as lean_epilogue_choice, plus 'a_scale' (BatchNorm in the operand path)"""
    M = sum(c.M for c in p.cls)
    cfg, bm, bn = pick_tile_x3f(tile_cfg, M, p.Cout, len(p.cls), stream_bn(p, ops))
    blocks = sum(-(-c.M // bm) for c in p.cls)
    epi = x3f_epilogue(p, ops)
    abn = 'a_scale' in ops and epi != 2
    if cfg == 5:
        return ('x3f_stream', bn, epi, abn), bm, blocks
    return ('x3f', cfg, epi, abn), bm, blocks


def x3f_lds_bytes(p, inst):
    """-> (dynamic LDS, threads, (grid x, grid y)) of an fp32-operand instantiation"""
    if inst[0] == 'x3f_stream':
        bn = inst[1]
        bm = 64 if bn == 256 else 128
        wgs, _ = stream_workgroups(p, bn)
        return stream_lds_bytes(bm, bn, 2, bn == 256, p.Cin), 64 * 2 * (2 if bn == 64 else 4), (wgs * (p.Cout // bn), 1)
    bm = 64 if inst[1] == 2 else 128
    return 2 * 3 * (bm + 64) * 32 * 2, 256, launch_grid(p, bm, 64)


def x3f_stat_blocks(B, H, W, cin, cout, k, stride, pad, tile_cfg):
    if not (k == 1 and pad == 0):
        return -1
    return x3f_route(fwd_problem(B, H, W, cin, cout, k, stride, pad), tile_cfg, {'y', 'stats'})[2]


def dgrad_x3f_bn_blocks(B, H, W, cin, cout, k, stride, pad, tile_cfg):
    if not (k == 1 and pad == 0 and stride in (1, 2)):
        return -1
    return x3f_route(dgrad_problem(B, H, W, cin, cout, k, stride, pad), tile_cfg, {'y', 'bnr_raw'})[2]


# ------------------------------------------------------------------------------------------------------------------------------------
# weight gradients (conv_wgrad.hip, conv_wgrad_x3f.hip)

WPlan = namedtuple('WPlan', 'inst splits unit units tiles taps')      # unit: rows (pixels) or chunks per split; units: M or nchunks


def wgrad_big_tile(M, cin, cout, taps):
    return cin % 128 == 0 and cout % 128 == 0 and taps == 1 and M >= 8192


def wgrad_splits(M, tiles, big=False, x3=False):
    s = ((256 if x3 else 512) if big else 1536)
    s = (s + tiles - 1) // tiles
    return max(1, min(s, (M + 127) // 128))


def wgrad3_plan(B, h, w, cin, cout, k, stride, pad, cp=32):
    """halo-patch plan -> None (the layer takes the per-tap kernel) or (nchunks, chunks_per_split, splits)"""
    if not (k == 3 and stride == 1 and pad == 1):
        return None
    if w < 8 or (w & (w - 1)):
        return None
    cw = w if w < 32 else 32
    rpc = cp // cw
    if h % rpc:
        return None
    nchunks = B * (h // rpc) * (w // cw)
    tiles = (cout // 64) * (cin // 64)
    s = max(1, min((256 + tiles - 1) // tiles, (nchunks + 3) // 4))
    cps = (nchunks + s - 1) // s
    return nchunks, cps, (nchunks + cps - 1) // cps


def wgrad_x3_route(B, h, w, cin, cout, k, stride, pad):
    """1 halo-patch kernel on the planes, 2 per-tap kernel on the planes, 0 the fp32 kernels"""
    if wgrad3_plan(B, h, w, cin, cout, k, stride, pad):
        return 1
    return 2 if (k * k > 1 or (cin >= 128 and cout >= 128)) else 0


def wgrad_x3_block(M, cin, cout, taps, big, stride):
    bco = bci = 128 if big else 64
    if taps == 1:
        if M >= 32768 and cout % 256 == 0 and cin % 128 == 0:
            bco, bci = 256, 128
        elif M <= 8192 and cout % 128 == 0 and cin % 128 == 0:
            bco, bci = (64, 128) if (stride == 1 and cout > cin) else (128, 64)
    elif cout % 256 == 0 and cin % 128 == 0:
        bco, bci = 256, 128
    elif cout % 128 == 0 and cin % 64 == 0:
        bco, bci = 128, 64
    return bco, bci


def _rows_per_split(M, splits):
    return ((M + splits - 1) // splits + 31) // 32 * 32


def wgrad_plan(B, h, w, cin, cout, k, stride, pad, planes=True):
    """what straps_conv_wgrad_x3 (planes given / not given = straps_conv_wgrad) launches -> WPlan"""
    taps = k * k
    route = wgrad_x3_route(B, h, w, cin, cout, k, stride, pad) if planes else 0
    p3 = wgrad3_plan(B, h, w, cin, cout, k, stride, pad)
    if p3 and route in (0, 1):
        nchunks, cps, s3 = p3
        if route == 0:
            return WPlan(('wgrad3_f32',), s3, cps, nchunks, (cout // 64) * (cin // 64), 9)
        p64 = wgrad3_plan(B, h, w, cin, cout, k, stride, pad, 64)
        if p64 and p64[2] <= s3:
            return WPlan(('wgrad3_x3', 64), p64[2], p64[1], p64[0], (cout // 64) * (cin // 64), 9)
        return WPlan(('wgrad3_x3', 32), s3, cps, nchunks, (cout // 64) * (cin // 64), 9)
    ho, wo = out_hw(h, w, k, stride, pad)
    M = B * ho * wo
    big = wgrad_big_tile(M, cin, cout, taps)
    if route == 0:
        t = 128 if big else 64
        tiles = taps * (cout // t) * (cin // t)
        s = wgrad_splits(M, tiles, big)
        return WPlan(('wgrad_f32', t), s, _rows_per_split(M, s), M, tiles, taps)
    bco, bci = wgrad_x3_block(M, cin, cout, taps, big, stride)
    tiles = taps * (cout // bco) * (cin // bci)
    if bco == bci:
        s = wgrad_splits(M, tiles, bco == 128, True)
    else:
        lds = 2 * 3 * 32 * (bco + bci) * 2
        per_cu = max(1, (160 * 1024) // lds)
        s = (256 * per_cu + tiles - 1) // tiles
        s = min(s, (M + 127) // 128)
        t = 128 if big else 64
        s = max(1, min(s, wgrad_splits(M, taps * (cout // t) * (cin // t), big)))
    return WPlan(('wgrad_x3', bco, bci), s, _rows_per_split(M, s), M, tiles, taps)


def wgrad_clamp(B, h, w, cin, cout, k, stride, pad):
    """which bound decides the split count of a per-tap plan on the planes: 'target' (workgroups per launch / tiles), 'max_s' = (M + 127) / 128, or
    'cap' = the fp32 plan's count, by which the shared workspace is sized (rectangular blocks only)"""
    ho, wo = out_hw(h, w, k, stride, pad)
    M, taps = B * ho * wo, k * k
    pl = wgrad_plan(B, h, w, cin, cout, k, stride, pad)
    assert pl.inst[0] == 'wgrad_x3'
    big = wgrad_big_tile(M, cin, cout, taps)
    t = 128 if big else 64
    cap = wgrad_splits(M, taps * (cout // t) * (cin // t), big)
    if pl.inst[1] != pl.inst[2]:
        lds = 2 * 3 * 32 * (pl.inst[1] + pl.inst[2]) * 2
        target = (256 * max(1, (160 * 1024) // lds) + pl.tiles - 1) // pl.tiles
    else:
        target, cap = ((256 if pl.inst[1] == 128 else 1536) + pl.tiles - 1) // pl.tiles, 1 << 30
    max_s = (M + 127) // 128
    assert pl.splits == max(1, min(target, max_s, cap))
    return 'target' if target <= min(max_s, cap) else 'max_s' if max_s <= cap else 'cap'


def wgrad_workspace_bytes(B, h, w, cin, cout, k, stride, pad):
    """straps_conv_wgrad_workspace_bytes: the fp32 plan's"""
    pl = wgrad_plan(B, h, w, cin, cout, k, stride, pad, planes=False)
    return pl.splits * cout * pl.taps * cin * 4


def wgrad_x3f_block(cin, cout):
    if cout % 256 == 0 and cin == 64:
        return 256, 64
    if cin % 256 == 0 and cout == 64:
        return 64, 256
    if cout % 256 == 0 and cin % 128 == 0 and cout >= cin:
        return 256, 128
    if cin % 256 == 0 and cout % 128 == 0:
        return 128, 256
    if cout % 128 == 0 and cin % 128 == 0:
        return 128, 128
    return 64, 64


def wgrad_x3f_plan(B, h, w, cin, cout, stride, abn=False):
    M = B * ((h - 1) // stride + 1) * ((w - 1) // stride + 1)
    bco, bci = wgrad_x3f_block(cin, cout)
    tiles = (cout // bco) * (cin // bci)
    s = ((512 if (bco, bci) == (64, 64) else 256) + tiles - 1) // tiles
    s = max(1, min(s, (M + 63) // 64))
    return WPlan(('wgrad_x3f', bco, bci, bool(abn)), s, _rows_per_split(M, s), M, tiles, 1)


def wgrad_x3f_workspace_bytes(B, h, w, cin, cout, k, stride, pad):
    if k != 1 or pad != 0 or stride < 1 or cin % 64 or cout % 64:
        return 0
    return wgrad_x3f_plan(B, h, w, cin, cout, stride).splits * cout * cin * 4


def last_split_state(pl):
    """'full' / 'short' / 'empty': what the round-up of the per-split extent leaves the last split of a plan"""
    left = pl.units - (pl.splits - 1) * pl.unit
    return 'empty' if left <= 0 else 'short' if left < pl.unit else 'full'


# ------------------------------------------------------------------------------------------------------------------------------------
# the single-product bf16 inference route (conv_bf16.hip): the PL != 0 instantiations of conv_x3_kernels.h with the EPI = 3 plane epilogue

BF16_BM = {1: 128, 2: 128, 3: 64, 4: 256, 5: 256, 6: 128, 7: 128, 8: 128, 9: 128, 10: 128}
BF16_BN = {1: 128, 2: 64, 3: 64, 4: 128, 5: 128, 6: 128, 7: 128, 8: 64, 9: 128, 10: 64}
BF16_PL = {1: 2, 2: 2, 3: 2, 4: 2, 5: 2, 6: 4, 7: 2, 8: 1, 9: 2, 10: 2}          # 32-channel K chunks per stage
BF16_NST = {1: 3, 2: 3, 3: 3, 4: 2, 5: 2, 6: 2, 7: 3, 8: 3, 9: 3, 10: 2}         # stages of the operand ring
BF16_PIPE = (5, 7)                                                              # the software-pipelined loop: its prologue issues NST chunks
BF16_HALO = {9: 208, 10: 272}                                                   # the halo-patch tiles and their slot limits
BF16_TILES = tuple(sorted(BF16_BM))
# what cfg_refusal says (the texts of straps_last_error(), as far as a test needs to tell them apart)
BF16_WHY_N = "cout is not a multiple of the tile's N extent"
BF16_WHY_K = 'the four-chunk stage needs cin % 128 == 0'
BF16_WHY_HALO = {9: 'the halo-patch tile needs a 3x3 / stride-1 layer whose patch fits 208 slots', 10: 'the halo-patch tile needs a 3x3 / stride-1 layer whose patch fits 272 slots'}


def pick_tile_bf16(M, cout):
    """conv_bf16.hip's pick_tile_bf16: the configuration tile_cfg = 0 takes"""
    t128 = ((M + 127) // 128) * (cout // 128)
    if cout % 128 != 0 or t128 < 256:
        return 3
    return 1 if t128 < 512 else 5


def bf16_refusal(p, cfg):
    """conv_bf16.hip's cfg_refusal -> None (the problem admits the configuration) or the reason"""
    if cfg not in BF16_BM:
        return 'unknown tile configuration'
    if p.Cout % BF16_BN[cfg] != 0:
        return BF16_WHY_N
    if cfg == 6 and p.Cin % 128 != 0:
        return BF16_WHY_K
    if cfg in BF16_HALO and not 0 < halo_patch_slots(p) <= BF16_HALO[cfg]:
        return BF16_WHY_HALO[cfg]
    return None


def bf16_route(p, cfg):
    """-> ('bf16', cfg): the instantiation dispatch_bf16 launches for an ADMITTED configuration (cfg 0: the automatic rule's)"""
    if cfg == 0:
        cfg = pick_tile_bf16(p.cls[0].M, p.Cout)
    assert bf16_refusal(p, cfg) is None, (p, cfg)
    return ('bf16', cfg)


def bf16_lds_bytes(cfg):
    """(dynamic LDS, threads): the plane kernels' formula with PL chunks of one plane in the three planes' place"""
    pl, nst, bm, bn = BF16_PL[cfg], BF16_NST[cfg], BF16_BM[cfg], BF16_BN[cfg]
    if cfg in BF16_HALO:
        return ((2 if cfg == 9 else 1) * pl * BF16_HALO[cfg] + nst * pl * bn) * 32 * 2, 256
    return nst * pl * (bm + bn) * 32 * 2, 512 if bm == 256 else 256


def bf16_nchunks(p, cfg):
    """stages of the K loop: taps x (32-channel chunks / PL) -- the kernels' nchunks / nsteps"""
    return p.cls[0].ntaps * ((p.Cin // 32) // BF16_PL[cfg])


def bf16_problem(c):
    B, H, W, ci, co, k, s = c[:7]
    return fwd_problem(B, H, W, ci, co, k, s, k // 2)


# A bf16 case is (B, H, W, Cin, Cout, k, stride), pad = k // 2.  BF16_EXPLICIT: every case runs under EVERY configuration 1..10 -- launched where
# bf16_refusal admits it, refused with the stated reason elsewhere.  BF16_AUTO: tile_cfg = 0.
BF16_KLOOP = [(1, 5, 13, ci, 128, 1, 1) for ci in (64, 128, 192, 256, 384)] + \
             [(2, 9, 9, 64, 128, 3, 1), (2, 9, 9, 128, 128, 3, 1)]      # 3x3: the tap rolls over every stage (cin 64, PL = 2) / every second one
# M = 1, BM - 1, BM, BM + 1 and a ragged two-tile M for BM = 64, 128, 256 (1x1, cin 64): M = 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385
BF16_M_EDGES = [(1, 1, 1, 64, 64, 1, 1)] + [(1, h, w, 64, 128, 1, 1) for (h, w) in ((1, 1), (1, 63), (8, 8), (65, 1), (1, 127), (1, 128), (1, 129), (3, 85), (16, 16), (257, 1), (5, 77))]
# 3x3 whose taps are all padding but the centre (H = W = 1) / but the centre row (H = 1): every PL slot of a padding pixel reads the zero constant
BF16_PADDING = [(1, 1, 1, 64, 128, 3, 1), (1, 1, 3, 64, 128, 3, 1), (1, 1, 1, 128, 128, 3, 1), (1, 1, 3, 128, 128, 3, 1)]
BF16_STRIDE2 = [(3, 7, 9, 64, 128, 3, 2), (2, 7, 5, 128, 64, 1, 2)]
BF16_N_EDGES = [(1, 5, 13, 64, 64, 1, 1), (1, 5, 13, 64, 192, 1, 1), (1, 5, 13, 64, 320, 1, 1), (2, 9, 9, 64, 192, 3, 1)]
# halo tiles: a patch of two images (200 slots), one image per tile (180), two tiles per image (180), four-row tiles (204); 264 slots: cfg 10 alone
BF16_HALO_RUN = [(b, h, w, ci, 128, 3, 1) for (b, h, w) in ((2, 8, 8), (1, 16, 8), (1, 16, 16), (1, 32, 32)) for ci in (64, 128)] + \
                [(1, 64, 64, 64, 64, 3, 1), (1, 64, 64, 64, 128, 3, 1)]
# ... and refused by both: 288 slots, a stride-2 layer, a 1x1 layer, M % 128 != 0
BF16_HALO_REFUSED = [(8, 4, 4, 64, 128, 3, 1), (2, 16, 16, 64, 128, 3, 2), (2, 8, 8, 64, 128, 1, 1), (3, 8, 8, 64, 128, 3, 1)]
# the ragged geometries of tests/test_gpu_conv_bf16.py::test_ragged_tiles_and_output_forms (the first is in BF16_STRIDE2)
BF16_OLD_RAGGED = [(2, 5, 11, 128, 64, 1, 1), (1, 9, 9, 256, 128, 3, 1), (5, 8, 8, 512, 512, 3, 1)]
BF16_EXPLICIT = BF16_KLOOP + BF16_M_EDGES + BF16_PADDING + BF16_STRIDE2 + BF16_N_EDGES + BF16_HALO_RUN + BF16_HALO_REFUSED + BF16_OLD_RAGGED

# the automatic rule reads M and cout only: t128 = 255 / 256 / 511 / 512 -> cfg 3 / 1 / 1 / 5; 64 and 192 output channels stay on cfg 3 at 512 M tiles
# (cout = 192: t128 = 512, the `cout % 128` test comes first)
BF16_AUTO = [(1, 255, 128, 64, 128, 1, 1), (1, 256, 128, 64, 128, 1, 1), (1, 511, 128, 64, 128, 1, 1), (1, 512, 128, 64, 128, 1, 1),
             (1, 512, 128, 64, 64, 1, 1), (1, 512, 128, 64, 192, 1, 1)]
BF16_AUTO_WANT = [3, 1, 1, 5, 3, 3]

# a body alone equals its rows in the batch, bit for bit: (case, configuration) -- one 128-row tile spans all three images; a halo patch of two images
BF16_BATCH = [((3, 5, 5, 128, 128, 3, 1), 1), ((3, 5, 5, 128, 128, 3, 1), 7), ((2, 8, 8, 64, 128, 3, 1), 9)]

# split and pack: (rows, c) of straps_split_bf16_cm, (cout, cin, kh, kw) of straps_pack_conv_weight_bf16.  Both kernels run at most 16384 workgroups of
# 256 threads; split1_cm_kernel handles four values per thread, pack_w_bf16_kernel one
BF16_GRID_CAP = 16384 * 256
BF16_SPLIT = [(1, 32), (1, 64), (3, 96), (257, 32), (65536, 256), (65540, 256)]          # the last two: just under (exactly at) and just past the cap
BF16_PACK = [(64, 32, 1, 1), (64, 64, 3, 3), (192, 96, 3, 3), (1, 32, 3, 3), (64, 64, 1, 3), (64, 64, 3, 1), (512, 1024, 3, 3)]


def bf16_case_id(c):
    return 'B%d_%dx%d_%dto%d_k%ds%d' % tuple(c[:7])


# ------------------------------------------------------------------------------------------------------------------------------------
# the case tables.  A convolution case is (B, H, W, Cin, Cout, k, stride, tile_cfg): H x W is the INPUT map of the forward convolution (= the map of
# dx for a data gradient), Cin -> Cout its channels; pad = 1 for 3x3, 0 for 1x1.

def pad_of(k):
    return 1 if k == 3 else 0


def _in_map(oh, ow, stride):
    """input map whose 3x3 / pad 1 (or 1x1) stride-`stride` output is oh x ow (odd extents at stride 2)"""
    return (oh, ow) if stride == 1 else (2 * oh - 1, 2 * ow - 1)


# output maps (B, Ho, Wo) per row tile BM: M = BM + 1, M = 2 BM - 1, M < BM / 2 -- with H = 1 and W = 1 maps among them (a whole tap row / column of a
# 3x3 / pad 1 filter lies outside the map)
EDGE_MAPS = {
    64: ((1, 5, 13), (1, 127, 1), (1, 1, 31)),
    128: ((1, 3, 43), (1, 255, 1), (3, 1, 21)),
    256: ((1, 1, 257), (1, 7, 73), (5, 25, 1)),
}
# the four filter variants of every explicit tile: (k, stride, channels on the reduction side)
VARIANTS = ((3, 1, 32), (1, 1, 32), (1, 1, 64), (3, 2, 32))


def _explicit_fwd():
    out = []
    for cfg in X3_TILES:
        for k, stride, cin in VARIANTS:
            for (b, oh, ow) in EDGE_MAPS[X3_BM[cfg]]:
                h, w = _in_map(oh, ow, stride)
                out.append((b, h, w, cin, X3_BN[cfg], k, stride, cfg))
    return out


def _explicit_dgrad():
    """the same rows as gradients: the map is dx's; at stride 2 its largest parity class -- even rows and columns -- has the row's M, the other classes are smaller"""
    out = []
    for cfg in X3_TILES:
        for k, stride, cred in VARIANTS:
            for (b, oh, ow) in EDGE_MAPS[X3_BM[cfg]]:
                h, w = _in_map(oh, ow, stride)
                out.append((b, h, w, X3_BN[cfg], cred, k, stride, cfg))
    return out


FWD_EXPLICIT = _explicit_fwd()
DGRAD_EXPLICIT = _explicit_dgrad()

# automatic rule, training forward (raw + statistics: lean EPI 1) and its fused-epilogue twin (shared epilogue on the same rule)
FWD_AUTO = [
    # Cout = 128, Cin = 32, 3x3 / stride 1: one row short of and one row past a tile multiple in each size class
    (1, 129, 127, 32, 128, 3, 1, 0), (5, 29, 113, 32, 128, 3, 1, 0),          # tile 7: 128 <= t128 < 256 (M = 16 383, 16 385)
    (7, 31, 151, 32, 128, 3, 1, 0), (9, 11, 331, 32, 128, 3, 1, 0),           # tile 5: 256 <= t128 < 512, ragged: no halo (M = 32 767, 32 769)
    (15, 17, 257, 32, 128, 3, 1, 0), (3, 91, 241, 32, 128, 3, 1, 0),          # tile 12: t128 >= 512 (M = 65 535, 65 793 = 257 x 256 + 1)
    (1, 5, 13, 32, 128, 3, 1, 0), (1, 129, 127, 32, 128, 1, 1, 0),            # tile 3: fewer than 128 tile equivalents; tile 7 with ONE K chunk
    # halo 1: M % 128 == 0, 256 <= t128 < 512, at most 208 patch slots: four-row tiles of a 32-wide map, two whole 8x8 images per tile
    (32, 32, 32, 32, 128, 3, 1, 0), (512, 8, 8, 32, 128, 3, 1, 0),
    # Cout = 64: ragged -> tile 11; halo 3 (single patch buffer) at the smallest whole-image tile, at a two-row tile, one channel chunk (no patch
    # reload) and four (three reloads)
    (1, 3, 43, 32, 64, 3, 1, 0), (3, 5, 17, 32, 64, 3, 1, 0), (1, 1, 31, 32, 64, 3, 1, 0), (1, 3, 43, 64, 64, 1, 1, 0),
    (4, 4, 8, 32, 64, 3, 1, 0), (1, 4, 64, 32, 64, 3, 1, 0), (1, 4, 64, 128, 64, 3, 1, 0), (2, 8, 8, 128, 64, 3, 1, 0),
    # halo 2 (two patch buffers, 64-channel outputs) only through bit 9; bit 9 also takes halo 1 below 256 tile equivalents
    (1, 4, 64, 32, 64, 3, 1, 512), (2, 8, 8, 64, 64, 3, 1, 512), (4, 8, 8, 32, 128, 3, 1, 512),
]

# straps_conv_fwd_x3p (the result's planes from the epilogue): the 64x64 tile and one 128-wide tile, ragged M
FWD_PLANES = [(1, 5, 13, 32, 64, 3, 1, 3), (1, 3, 43, 32, 128, 3, 1, 1), (1, 3, 43, 64, 128, 1, 1, 1), (1, 1, 31, 32, 64, 3, 1, 3)]

# stride-2 data gradients at tiny maps: one, two and four parity classes, dead classes of a 1x1 filter, a ragged class
DGRAD_S2_SMALL = [(2, h, w, 64, 32, k, 2, 0) for k in (3, 1) for (h, w) in ((1, 1), (1, 2), (2, 1), (3, 3), (2, 5))] + \
                 [(3, 9, 13, 64, 64, 1, 2, 3), (3, 9, 13, 128, 32, 1, 2, 1)]

# automatic rule, data gradients (lean EPI 2 with an addend / ReLU bits / fused BatchNorm sums): the forward's size classes as gradients (Cin is the
# GEMM's column count here, Cout = 32 its reduction) ...
DGRAD_AUTO = [
    (1, 129, 127, 128, 32, 3, 1, 0), (7, 31, 151, 128, 32, 3, 1, 0), (3, 91, 241, 128, 32, 3, 1, 0),      # tiles 7, 5, 12
    (32, 32, 32, 128, 32, 3, 1, 0),                                                                       # halo 1
    (4, 4, 8, 64, 32, 3, 1, 0), (1, 4, 64, 64, 128, 3, 1, 0),                                             # halo 3, one chunk / three reloads
    (1, 3, 43, 64, 32, 3, 1, 0), (1, 5, 13, 128, 32, 3, 1, 0),                                            # tiles 11 and 3
    # ... and the stride-2 classes, a ragged class each (t = 128x128-tile equivalents per class): t < 128 -> 64x64; 128 <= t < 256 -> tile 11;
    # 256 <= t < 512 -> tile 9 for a one-tap filter, tile 12 for 3x3; t >= 512 -> tile 12
    (2, 9, 14, 128, 32, 3, 2, 0), (1, 255, 257, 128, 32, 3, 2, 0), (1, 255, 257, 256, 32, 3, 2, 0), (1, 255, 257, 256, 32, 1, 2, 0),
    (1, 255, 257, 512, 32, 3, 2, 0),
]

# the fp32-operand route: (B, H, W, Cin, Cout, stride, tile_cfg), 1x1 filters; the reduction side at 64 channels
X3F_FWD = [
    (1, 5, 13, 64, 64, 1, 2), (1, 7, 9, 64, 64, 1, 2), (1, 3, 43, 64, 64, 1, 1), (1, 127, 1, 64, 128, 1, 1), (1, 9, 13, 64, 64, 2, 1), (2, 11, 7, 64, 128, 2, 2),
    (1, 5, 13, 64, 64, 1, 0), (1, 3, 43, 64, 256, 1, 0),
    # streaming kernel: fewer tiles than workgroups (64 / 128 / 256 wide), one tile more than a multiple of its grid, by rule (tile_cfg 0) and by name
    (1, 3, 43, 64, 64, 1, 5), (1, 3, 43, 64, 128, 1, 5), (1, 5, 13, 64, 256, 1, 5), (1, 9, 13, 64, 64, 2, 5),
    (5, 116, 113, 64, 64, 1, 5), (1, 127, 259, 64, 128, 1, 5), (5, 29, 113, 64, 256, 1, 5),          # 513 = 512 + 1, 257 = 256 + 1 (twice) tiles
    (1, 257, 255, 64, 64, 1, 0), (1, 129, 127, 64, 256, 1, 0),          # the size rule of the two plain tiles
    (9, 11, 331, 64, 1024, 1, 0),          # the streaming kernel BY RULE: at least four 128-row tiles per workgroup (M = 32 769)
]
X3F_DGRAD = [      # (B, H, W, Cin, Cout, stride, tile_cfg): the gradient's reduction runs over Cout = 64
    (1, 5, 13, 64, 64, 1, 2), (1, 3, 43, 64, 64, 1, 1), (1, 127, 1, 128, 64, 1, 1), (1, 9, 13, 64, 64, 2, 1), (2, 11, 7, 128, 64, 2, 2), (1, 2, 5, 64, 64, 2, 0),
    (1, 5, 13, 64, 64, 1, 0), (1, 3, 43, 64, 64, 1, 5), (1, 3, 43, 128, 64, 1, 5), (1, 5, 13, 256, 64, 1, 5),
    (1, 257, 255, 64, 64, 1, 0), (1, 129, 127, 256, 64, 1, 0),
    (5, 29, 113, 256, 64, 1, 5), (1, 127, 259, 128, 64, 1, 5), (5, 116, 113, 64, 64, 1, 5),          # one tile more than the grid: 256, 128, 64 wide
    (9, 11, 331, 1024, 64, 1, 0),          # the streaming kernel by rule
]

# weight gradients: (B, H, W, Cin, Cout, k, stride)
WGRAD_HALO = [
    (1, 4, 8, 64, 64, 3, 1),          # W = 8: one chunk, one split; the 64-pixel plan needs H % 8 == 0: refused
    (1, 8, 8, 64, 64, 3, 1),          # the 64-pixel plan at its smallest: one chunk
    (3, 2, 16, 64, 64, 3, 1), (3, 4, 16, 64, 128, 3, 1),          # W = 16: two rows per chunk (four in the 64-pixel plan)
    (5, 3, 32, 64, 64, 3, 1), (5, 6, 32, 128, 64, 3, 1),          # W = 32: one row per chunk; an odd H: 32-pixel plan only
    (3, 3, 64, 64, 64, 3, 1), (7, 2, 64, 64, 64, 3, 1),           # W = 64: two chunks per row; nchunks no multiple of chunks_per_split
    (9, 2, 32, 64, 64, 3, 1),          # nine 64-pixel chunks in three splits against eighteen 32-pixel ones in five
    (13, 8, 8, 64, 64, 3, 1),          # 64-pixel plan, nchunks = 13: splits of 4, 4, 4, 1 chunks
]
# per-tap kernel on the planes: every block of wgrad_x3_block at M in {1, 31, 33, 129} where its rule admits them (the 1x1 rules have pixel-count
# thresholds), a short last split, an empty last split, each clamp of the split count
WGRAD_TAP = [(1, h, w, ci, co, 3, 2) for (ci, co) in ((128, 256), (64, 128), (64, 64)) for (h, w) in ((1, 1), (1, 61), (5, 21), (5, 85))] + \
            [(1, h, w, ci, co, 1, 1) for (ci, co) in ((128, 256), (256, 128)) for (h, w) in ((1, 1), (1, 31), (3, 11), (3, 43))] + [
    (2, 10, 24, 64, 64, 3, 1), (1, 9, 16, 64, 128, 3, 1),                       # 3x3 / stride 1 outside the halo plan (width 24, rows that do not fill a chunk)
    (1, 91, 91, 128, 128, 1, 1), (1, 64, 129, 128, 128, 1, 1),                  # 128 x 128: 1x1 with more than 8 192 pixels
    (2, 128, 128, 128, 256, 1, 1), (1, 181, 182, 128, 256, 1, 1),               # 256 x 128 by the 1x1 rule: >= 32 768 pixels
    (1, 7, 11, 192, 128, 1, 1), (3, 20, 20, 384, 256, 1, 1),                    # 64 x 64 for a 1x1 layer: a side that is no multiple of 128
    (1, 33, 33, 128, 256, 3, 2), (1, 19, 27, 128, 256, 3, 2), (1, 41, 41, 64, 128, 3, 2), (1, 45, 45, 64, 64, 3, 2),
    (1, 64, 65, 256, 128, 1, 1), (1, 64, 128, 128, 256, 1, 1),
    # the split count at its TARGET (or, 256 x 128 under a 3x3 filter, at the fp32 plan's count, the `cap`) instead of at (M + 127) / 128: the round-up of
    # the rows per split to 32 then leaves the last splits EMPTY -- they must still write their zeros, the reduction reads them
    (1, 147, 150, 64, 64, 3, 1), (1, 147, 199, 64, 128, 3, 2), (1, 99, 115, 128, 256, 3, 2), (1, 42, 100, 256, 512, 1, 1), (1, 42, 100, 512, 256, 1, 1),
    (1, 150, 220, 128, 128, 1, 1),
]
# the fp32 kernels (straps_conv_wgrad; straps_conv_wgrad_x3 without planes): both square blocks, the fp32 halo kernel
WGRAD_F32 = [(1, 4, 8, 64, 64, 3, 1), (7, 2, 64, 64, 64, 3, 1), (1, 1, 1, 64, 64, 3, 2), (1, 3, 43, 64, 128, 1, 1), (1, 5, 21, 64, 64, 3, 2), (1, 91, 91, 128, 128, 1, 1),
             (1, 3, 11, 128, 64, 1, 2)]
# the fp32-operand weight gradient: (B, H, W, Cin, Cout, stride, operand-path BatchNorm): every block at M in {1, 31, 33, 129}, ragged and clamped splits
WGRAD_X3F = [(1, h, w, ci, co, 1, bn) for (ci, co, bn) in ((64, 256, 1), (256, 64, 0), (128, 256, 1), (256, 128, 0), (128, 128, 1), (64, 64, 0))
             for (h, w) in ((1, 1), (1, 31), (3, 11), (3, 43))] + [
    (1, 7, 19, 64, 256, 1, 0), (1, 13, 25, 256, 64, 2, 1), (2, 9, 9, 128, 256, 2, 0), (1, 65, 65, 64, 64, 1, 1), (1, 33, 31, 128, 128, 1, 0), (1, 5, 13, 256, 128, 1, 1),
    (1, 32, 33, 512, 512, 1, 0), (1, 42, 50, 512, 512, 1, 0),          # eight tiles: (M + 63) / 64 decides; the target of 32 splits decides, the last ones empty
]


def fwd_ops(variant):
    return {'raw_stats': {'y', 'stats'}, 'fused': {'y', 'scale', 'res', 'relu'}, 'planes': {'y', 'scale', 'res', 'relu', 'yplanes'},
            'planes_only': {'scale', 'res', 'relu', 'yplanes'}}[variant]


DGRAD_FORMS = {      # operands of a data-gradient call by the form's name
    'plain': {'y'}, 'addend': {'y', 'res'}, 'bits': {'y', 'res', 'res_bits'},
    'bn_out': {'y', 'res', 'bnr_raw', 'bnr_out'}, 'bn_mask': {'y', 'res', 'bnr_raw'}, 'bn_bits': {'y', 'res', 'res_bits', 'bnr_raw'},
    'bn_noadd': {'y', 'bnr_raw'},
}


# ---- what tests/test_gpu_conv_edges.py runs per case: the GPU file iterates over these lists and reached() below counts from the same ones
FWD_RUN = ('raw_stats', 'fused')          # forms of a plane-route forward case; a lean launch runs again under twin_cfg
X3F_FWD_FORMS = {      # forms of an fp32-operand forward case: operands of the launch
    'raw_stats': {'y', 'stats'}, 'abn_stats': {'y', 'stats', 'a_scale'},
    'eval': {'y', 'scale', 'res', 'relu'}, 'abn_eval': {'y', 'scale', 'res', 'relu', 'a_scale'},
}
X3F_DGRAD_FORMS = {'plain': {'y'}, 'full': {'y', 'res', 'res_bits', 'bnr_raw'}}


def dgrad_is_big(c):
    """the large automatic-rule gradients (more than 2^22 elements of dx) run a shorter list of forms"""
    return c[0] * c[1] * c[2] * c[3] > (1 << 22)


def dgrad_run(c):
    """-> [(form of DGRAD_FORMS, whether a lean launch of it runs again under twin_cfg)] in the order the GPU test runs them"""
    if dgrad_is_big(c):
        return [('plain', True), ('addend', True), ('bits', False), ('bn_out', False), ('bn_bits', False), ('bn_mask', True)]
    return [('plain', True), ('addend', True), ('bits', False), ('bn_out', False), ('bn_bits', True), ('bn_mask', True), ('bn_noadd', True)]


def x3f_case_id(c):
    return 'B%d_%dx%d_%dto%d_s%d_cfg%d' % c


def conv_case_id(c):
    return 'B%d_%dx%d_%dto%d_k%ds%d_cfg%d' % c


def _problem(kind, g):
    return (fwd_problem if kind == 'fwd' else dgrad_problem)(*g)


def restated_inst(route, kind, g, cfg, ops):
    """the instantiation a launch reaches by the restatement.  route: 'x3' / 'x3f' / 'bf16'; kind: 'fwd' / 'dgrad'; g = (B, H, W, Cin, Cout, k, stride, pad)"""
    p = _problem(kind, g)
    return {'x3': x3_route, 'x3f': x3f_route}[route](p, cfg, ops)[0] if route != 'bf16' else bf16_route(p, cfg)


def launches():
    """every launch of the forward / data-gradient tables of tests/test_gpu_conv_edges.py and test_gpu_conv_bf16_edges.py, from the lists the GPU files
    themselves iterate over (FWD_RUN, dgrad_run(case), X3F_FWD_FORMS, X3F_DGRAD_FORMS; every admitted bf16 configuration):
    -> [(case id, route, kind, g, tile_cfg, ops, whether a lean launch runs again under its twin's tile_cfg)]"""
    out = []
    for c in FWD_EXPLICIT + FWD_AUTO:
        B, H, W, ci, co, k, s, cfg = c
        out += [('fwd:' + conv_case_id(c), 'x3', 'fwd', (B, H, W, ci, co, k, s, pad_of(k)), cfg, fwd_ops(v), True) for v in FWD_RUN]
    for c in FWD_PLANES:
        B, H, W, ci, co, k, s, cfg = c
        out += [('fwdp:' + conv_case_id(c), 'x3', 'fwd', (B, H, W, ci, co, k, s, pad_of(k)), cfg, fwd_ops(v), False) for v in ('planes', 'planes_only')]
    for c in DGRAD_EXPLICIT + DGRAD_S2_SMALL + DGRAD_AUTO:
        B, H, W, ci, co, k, s, cfg = c
        out += [('dgrad:' + conv_case_id(c), 'x3', 'dgrad', (B, H, W, ci, co, k, s, pad_of(k)), cfg, DGRAD_FORMS[form], with_twin) for form, with_twin in dgrad_run(c)]
    for c in X3F_FWD:
        B, H, W, ci, co, s, cfg = c
        out += [('x3f_fwd:' + x3f_case_id(c), 'x3f', 'fwd', (B, H, W, ci, co, 1, s, 0), cfg, ops, False) for ops in X3F_FWD_FORMS.values()]
    for c in X3F_DGRAD:
        B, H, W, ci, co, s, cfg = c
        out += [('x3f_dgrad:' + x3f_case_id(c), 'x3f', 'dgrad', (B, H, W, ci, co, 1, s, 0), cfg, ops, False) for ops in X3F_DGRAD_FORMS.values()]
    for c in BF16_EXPLICIT:
        p = bf16_problem(c)
        out += [('bf16:' + bf16_case_id(c), 'bf16', 'fwd', c + (c[5] // 2,), cfg, {'y', 'yplanes'}, False) for cfg in BF16_TILES if bf16_refusal(p, cfg) is None]
    out += [('bf16:' + bf16_case_id(c) + '_cfg0', 'bf16', 'fwd', c + (c[5] // 2,), 0, {'y', 'yplanes'}, False) for c in BF16_AUTO]
    return out


def reached(inst_of=restated_inst):
    """every instantiation the tables reach -> {instantiation: [case ids]}: launches() -- a lean plane launch again under its twin's tile_cfg --
    through inst_of (the restatement, or the library's plan: tests/test_conv_cases_cpu.py), and one plan per weight-gradient case"""
    got = {}

    def add(inst, cid):
        got.setdefault(inst, [])
        if cid not in got[inst]:
            got[inst].append(cid)

    for cid, route, kind, g, cfg, ops, with_twin in launches():
        inst = inst_of(route, kind, g, cfg, ops)
        add(inst, cid)
        if route == 'x3' and inst[2] and with_twin:
            add(inst_of(route, kind, g, twin_cfg(_problem(kind, g), cfg, ops), ops), cid)
    for c in WGRAD_HALO + WGRAD_TAP:
        add(wgrad_plan(*c, pad_of(c[5])).inst, 'wgrad:B%d_%dx%d_%dto%d_k%ds%d' % c)
    for c in WGRAD_F32:
        add(wgrad_plan(*c, pad_of(c[5]), planes=False).inst, 'wgrad_f32:B%d_%dx%d_%dto%d_k%ds%d' % c)
    for c in WGRAD_X3F:
        add(wgrad_x3f_plan(*c).inst, 'wgrad_x3f:B%d_%dx%d_%dto%d_s%d_bn%d' % c)
    return got


def twin_cfg(p, tile_cfg, ops):
    """tile_cfg under which the library runs the SAME tile / halo kernel with the shared epilogue (for a case the automatic rule gives a lean form):
    the tile named explicitly; a halo kernel has no number -- the shared-epilogue bit"""
    inst = x3_route(p, tile_cfg, ops)[0]
    assert inst[2] in (1, 2)
    return (tile_cfg | SHARED_EPILOGUE_BIT) if inst[0] == 'x3h' else inst[1]


# every instantiation the product library can dispatch to
REQUIRED = (
    [('x3', c, 0) for c in X3_TILES] + [('x3h', h, 0) for h in (1, 2, 3)] +
    [('x3', c, e) for c in LEAN_TILES for e in (1, 2)] + [('x3h', h, e) for h in (1, 3) for e in (1, 2)] +
    [('x3f', c, e, a) for c in (1, 2) for (e, a) in ((0, False), (0, True), (1, False), (1, True), (2, False))] +
    [('x3f_stream', bn, e, a) for bn in (256, 128, 64) for (e, a) in ((1, False), (1, True), (2, False))] +
    [('wgrad3_x3', 32), ('wgrad3_x3', 64), ('wgrad3_f32',), ('wgrad_f32', 64), ('wgrad_f32', 128)] +
    [('wgrad_x3', o, i) for (o, i) in ((256, 128), (128, 64), (64, 128), (128, 128), (64, 64))] +
    [('wgrad_x3f', o, i, a) for (o, i) in ((256, 64), (64, 256), (256, 128), (128, 256), (128, 128), (64, 64)) for a in (False, True)] +
    [('bf16', c) for c in BF16_TILES]
)

# instantiations the library holds that no 1x1 / 3x3 layer reaches (listed in DESIGN.md as well); the tables do not invent a route to them
UNREACHABLE = {
    ('x3', 9, 1): 'lean forward form on the eight-wave pipelined 128x128 tile: the rule picks tile 9 only for stride-2 gradients (several classes), the lean '
                  'forward form needs one class',
    ('x3', 9, 2): 'lean data-gradient form on tile 9: the rule picks tile 9 only for one-tap stride-2 gradients; those of a 1x1 filter have dead parity classes, '
                  'for which lean_epilogue_choice returns 0 (only a 2x2 / stride-2 filter, which no network here has, would give four one-tap classes)',
    ('wgrad_x3', 256, 64): 'conv_wgrad_x3_kernel<256, 64>: chosen by the tools build\'s tile switch only; wgrad_x3_block never returns it',
    ('wgrad_x3', 64, 256): 'conv_wgrad_x3_kernel<64, 256>: as above',
    ('wgrad_x3', 128, 256): 'conv_wgrad_x3_kernel<128, 256>: as above',
}
