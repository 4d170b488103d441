"""CPU: tests/head_cases.py -- the tables and float64 references of the IEF / pose / optimiser edge suites -- held together without a GPU:
every table reaches the edges it claims (the launch rules restated in head_cases.py, asserted per case), the references agree with independent
evaluations (torch.matmul, autograd of the oracle, torch.optim.Adam, F.mse_loss, the oracle's projections), the conditions on the data hold
(tracer sums below 2^24, the rot6d filter drops at most 5 %, no rodrigues row in the excluded neighbourhood unless marked), and the fp32-CPU
measurements that the projection tests multiply by 4 are computed and printed here.  The argument checks of straps_linear_fwd, straps_gemm_multi
and straps_orthographic_project_bwd return before any launch, so they are tested here as well, on the built library."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import head_cases as H
import straps_oracle as O
from straps_amd import hipabi


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


# ------------------------------------------------------------------------------------------------------------------------------------ tables

def test_linear_table_reaches_every_edge():
    assert {c.m for c in H.LINEAR} == set(H.LIN_M) and {c.n for c in H.LINEAR} == set(H.LIN_N) and {c.k for c in H.LINEAR} == set(H.LIN_K)
    r = H.linear_reach
    assert r(8) == (7, 1, False, True)                     # one group: seven waves idle
    assert r(56) == (1, 1, False, True)                    # seven groups
    assert r(64) == (0, 1, False, True)                    # exactly one group per wave
    assert r(72) == (0, 2, False, True)                    # one wave takes a second trip
    assert r(160) == (0, 3, False, True)
    assert r(520) == (0, 9, True, True)                    # 65 groups: the unrolled body twice, wave 0 a remainder trip
    assert r(2048) == (0, 32, True, False)                 # the unrolled body alone
    pairs = {(c.m, c.n) for c in H.LINEAR}
    assert {(33, 33), (1, 157), (1, 1), (31, 157), (70, 157), (33, 157), (31, 1), (70, 1)} <= pairs        # the tails combined
    assert {c.wpad for c in H.LINEAR} == {c.xpad for c in H.LINEAR} == {0, 4}
    assert {c.ldo for c in H.LINEAR if c.n == 157} == {157, 160} and all(c.ldo == c.n for c in H.LINEAR if c.n != 157)
    assert {c.bias for c in H.LINEAR} == {c.relu for c in H.LINEAR} == {c.addend for c in H.LINEAR} == {0, 1}
    assert {(c.relu, c.addend, c.bias) for c in H.LINEAR} >= {(1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 0)}
    assert all(c.k % 8 == 0 and (c.k + c.xpad) % 4 == 0 for c in H.LINEAR) and 18 <= len(H.LINEAR) <= 24


def test_gemm_table_reaches_every_edge():
    assert {c.k for c in H.GEMM} == set(H.GEMM_K) and {c.m for c in H.GEMM} == {c.n for c in H.GEMM} == set(H.GEMM_MN)
    r = H.gemm_reach
    assert r(1) == (1, True, True, True, 7) and r(3)[2:4] == (True, True) and r(4)[2:4] == (False, True) and r(5)[2:4] == (True, False)
    assert r(8) == (1, True, False, False, 7) and r(9) == (1, True, True, True, 6)
    assert r(64) == (1, True, False, False, 0)             # eight groups: every wave's second group lies beyond G
    assert r(65)[:2] == (1, True) and r(128) == (1, False, False, False, 0)       # sixteen groups: both halves of one trip, nothing beyond
    assert r(129) == (2, True, True, True, 0)              # the second trip of the outer loop
    assert r(136)[:2] == (2, True) and r(300) == (3, True, False, True, 0)
    assert {c.a for c in H.GEMM} == {'T', 'N', 'one'} and {c.b for c in H.GEMM} == {'nk', 'kn'}
    assert {(c.a, c.b) for c in H.GEMM} == {(a, b) for a in ('T', 'N', 'one') for b in ('nk', 'kn')}
    assert {c.acc for c in H.GEMM} == {0, 1} and {c.c2 for c in H.GEMM} == {0, 1, 2} and {c.addend for c in H.GEMM} == {c.mask for c in H.GEMM} == {0, 1}
    assert all(c.m == 1 for c in H.GEMM if c.a == 'one') and any(c.cpad for c in H.GEMM)
    first, last = H.GEMM[H.GEMM_MULTI[0]], H.GEMM[H.GEMM_MULTI[-1]]
    assert len(H.GEMM_MULTI) == 8 and (first.m, first.n, first.k) == (1, 1, 1) and (last.m, last.n, last.k) == (65, 65, 300)
    for c in H.GEMM:
        if c.mask:
            mk = H.gemm_data(c, 'real')['mask'].flatten()
            zero_bits = H.bits(mk)
            assert bool((mk > 0).any()) and bool((mk < 0).any()) or mk.numel() < 4
            assert bool(torch.isnan(mk).any()) or mk.numel() < 3
            assert int((zero_bits == 0).sum()) > 0 and (int((zero_bits == -2 ** 31).sum()) > 0 or mk.numel() < 2)
    masks = torch.cat([H.gemm_data(c, 'real')['mask'].flatten() for c in H.GEMM if c.mask])
    assert bool((masks > 0).any()) and bool((masks < 0).any()) and bool(torch.isnan(masks).any()) and int((H.bits(masks) == -2 ** 31).sum()) > 0


def test_pack_and_broadcast_tables():
    r = H.pack_reach
    assert [r(*p)[1] for p in H.PACK] == [False, False, True, False, False]
    assert r(*H.PACK[2])[0] == 2048 and H.pack_total(*H.PACK[2]) > 2048 * 256 > H.pack_total(*H.PACK[1])
    assert r(*H.PACK[3])[2] is False and r(*H.PACK[0])[2] is True and H.PACK[3][4] == H.PACK[3][1]
    for i in H.PACK_LINEAR:
        f, p, h1, h2, ld_e = H.PACK[i]
        assert h2 % 8 == 0 and p % 32 != 0                 # a valid kdim / ldw of straps_linear_fwd, and padding rows to rely on
    assert H.PACK[3][3] % 8 != 0                           # why the fourth case cannot be the weight of straps_linear_fwd
    sizes = [m * ld for cols, ld, m in H.BROADCAST]
    assert 255 in sizes and 258 in sizes and all(ld >= cols for cols, ld, m in H.BROADCAST) and any(ld == cols for cols, ld, m in H.BROADCAST)


def test_pose_tables():
    counts = [rows * per for rows, per, ld, ldd in H.ROT6D]
    assert {1, 255, 256, 257} <= set(counts) and {24, 264, 72} <= set(counts)
    assert any(ld != ldd for _, _, ld, ldd in H.ROT6D) and all(ld >= 6 * per + H.rot6d_offset(ld) and ldd >= 6 * per + H.rot6d_offset(ldd) for _, per, ld, ldd in H.ROT6D)
    assert set(H.RODRIGUES_N) == {1, 255, 256, 257}
    fams = {f for f, _ in H.rodrigues_specials()}
    assert fams == {'zero', 'small', 'pi', 'r10', 'r50'}
    for n in H.RODRIGUES_N:
        aa, fam = H.rodrigues_rows(n)
        assert aa.shape == (n, 3) and len(fam) == n
        ex = H.rodrigues_excluded(aa)
        assert all(f == 'zero' for f, e in zip(fam, ex.tolist()) if e), 'a row inside the excluded neighbourhood is not marked'
        if n > 1:
            assert set(fam) == fams | {'random'} and fam[-1] != 'random'
            assert bool((aa < 0).any(dim=0).all())         # negative axes
    r = H.ortho_bwd_reach
    assert r(1) == (1, 255, True, 3) and r(17)[3] == 3 and r(63) == (1, 193, True, 3) and r(64) == (1, 192, False, 3) and r(65)[3] == 2
    assert r(255) == (1, 1, True, 0) and r(256) == (1, 0, False, 0) and r(257) == (2, 0, True, 0) and r(513)[0] == 3 and r(6890) == (27, 0, True, 0)
    assert [(b * 31 + 255) // 256 for b in H.TARGETS_B] == [1, 1, 2, 9] and 8 * 31 == 248 and 9 * 31 == 279
    assert [(b * n + 255) // 256 for b, n in H.PERSP] == [1, 1, 2, 54] and 3 * 85 == 255 and 3 * 86 == 258


def test_optim_tables():
    a = {n: H.stride_reach(n, H.capped_grid(n)) for n in H.ADAM_N}
    assert a[1] == (1, False, True) and a[255] == (1, False, True) and a[256] == (1, False, False) and a[257] == (2, False, True)
    assert a[1048576] == (4096, False, False) and a[1048577] == (4096, True, True)          # 4096 blocks exactly; one element into the second trip
    f = {rc: H.stride_reach(rc[0] * rc[1], 256) for rc in H.MSE}
    assert f[(65535, 1)] == (256, False, True) and f[(65536, 1)] == (256, False, False) and f[(65537, 1)] == (256, True, True)
    assert 4681 * 14 == 65534 and f[(70, 216)][1] is False
    b = H.stride_reach(1048577, H.capped_grid(1048577))
    assert b == (4096, True, True) and all(not H.stride_reach(r * c, H.capped_grid(r * c))[1] for r, c in H.MSE)
    for rows, cols in H.MSE:
        _, _, half = H.mse_data(rows, cols, 'half', H.MSE_SCALES[0])
        _, _, one = H.mse_data(rows, cols, 'one_row', H.MSE_SCALES[0])
        assert int(one.sum()) == 1 and 1 <= int(half.sum()) <= rows and (rows < 7 or int(half.sum()) < rows)
    for step in H.ADAM_STEPS:
        p, g, m, v = H.adam_data(257, step)
        assert bool((g == 0).any()) and bool((g == 1e4).any()) and bool((g == H.f32(1e-20)).any()) and bool((v >= 0).all())
        assert (step == 1) == bool((m == 0).all() and (v == 0).all())
    assert float(torch.tensor(1e-20) ** 2) == 0.0 or float(torch.tensor(1e-20) ** 2) < 2.0 ** -126


# ------------------------------------------------------------------------------------------------------------------------------------ references

def test_gemm_references_against_matmul_and_tracer_sums_are_exact():
    for c in H.LINEAR:
        for kind in ('tracer', 'real'):
            x, w, bias, addend = H.linear_data(c, kind)
            assert w.shape[0] == (c.n + 31) // 32 * 32 and bool((w[c.n:, :c.k] == 0).all())
            want, pre, bound = H.linear_reference(c, x, w, bias, addend)
            mm = torch.matmul(x[:, :c.k].double(), w[:c.n, :c.k].double().t())
            if bias is not None:
                mm = mm + bias.double()
            if addend is not None:
                mm = mm + addend[:, :c.n].double()
            assert float((pre - mm).abs().max()) <= 1e-12 * max(1.0, float(mm.abs().max()))
            if kind == 'tracer':
                mag = x[:, :c.k].double().abs() @ w[:c.n, :c.k].double().abs().t()
                assert float(mag.max()) + 4 < 2 ** 24 and bool((pre == pre.round()).all())
                assert set(x[:, :c.k].flatten().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
                if c.relu:
                    assert bool((pre == 0).any()) and bool((pre < 0).any()), c        # exact zeros and negatives in the pre-activation
            else:
                fp32 = torch.matmul(x[:, :c.k], w[:c.n, :c.k].t())                    # an fp32 evaluation in another order meets the bound
                if bias is not None:
                    fp32 = fp32 + bias
                if addend is not None:
                    fp32 = fp32 + addend[:, :c.n]
                assert bool(((fp32.double() - pre).abs() <= bound).all())
    for c in H.GEMM:
        for kind in ('tracer', 'real'):
            d = H.gemm_data(c, kind)
            v, want, want2, b1, b2 = H.gemm_reference(c, d)
            mm = torch.matmul(d['A'].double(), d['B'].double())
            if d['addend'] is not None:
                mm = mm + d['addend'][:, :c.n].double()
            if d['mask'] is not None:
                mm = mm * (d['mask'] > 0)
            assert float((torch.nan_to_num(v) - mm).abs().max()) <= 1e-12 * max(1.0, float(mm.abs().max())) and bool(torch.isfinite(v).all())
            if kind == 'tracer':
                assert float((d['A'].double().abs() @ d['B'].double().abs()).max()) + 8 < 2 ** 24 and bool((want == want.round()).all())
            # the stored operands are the logical ones behind their strides
            a_flat, b_flat = d['a'].flatten(), d['b'].flatten()
            for (i, k, j) in ((0, 0, 0), (c.m - 1, c.k - 1, c.n - 1), (c.m // 2, c.k // 2, c.n // 2)):
                assert float(a_flat[i * d['sam'] + k * d['sak']]) == float(d['A'][i, k]) and float(b_flat[k * d['sbk'] + j * d['sbn']]) == float(d['B'][k, j])


def test_rot6d_formula_against_autograd_and_filter():
    worst_f = worst_b = 0.0
    for i, (rows, per, ld, ldd) in enumerate(H.ROT6D):
        x, dropped = H.rot6d_well_conditioned(rows, per, H.ROT6D_SEEDS[i])
        assert dropped <= 0.05, 'case %d: the filter replaced %.1f %% of the rotations' % (i, 100 * dropped)
        g = H.det((rows * per, 3, 3), 16 + i)
        R, dx = H.rot6d_autograd(x, g)
        Rf, dxf = H.rot6d_formula(x, g)
        assert float((R - Rf).abs().max()) < 1e-14 and float((dx - dxf).abs().max()) < 1e-12 * float(dx.abs().max())
        assert float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-14 and bool((torch.linalg.det(R) > 0).all())
        R32, dx32 = H.rot6d_formula(x, g, torch.float32)
        worst_f = max(worst_f, float((R32.double() - R).abs().max()))
        worst_b = max(worst_b, float(((dx32.double() - dx).abs().max(1).values / dx.abs().max(1).values).max()))
    print('MEASURED rot6d fp32 CPU evaluation: forward %.2e per element, backward %.2e of a rotation\'s largest entry' % (worst_f, worst_b))
    assert worst_f < 2e-6 and worst_b < 2e-5               # an honest fp32 evaluation meets the bars the kernel is held to
    x, dropped = H.rot6d_well_conditioned(257, 24, 15)     # the issue's figure: seed 15 keeps 96.8 % of 6168 rotations
    assert abs((1 - dropped) - 0.968) < 0.001


def test_rot6d_degenerate_reference_is_autograd_including_the_clamped_branches():
    deg = H.rot6d_degenerate()
    x = torch.stack([r for _, r, _ in deg])
    g = H.dyadic((len(deg), 3, 3), 41)
    R, dx = H.rot6d_autograd(x, g)
    Rf, dxf = H.rot6d_formula(x, g)
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(dx).all())
    exact = torch.tensor([e is True for _, _, e in deg])
    bwd = torch.tensor([e is True or e == 'bwd' for _, _, e in deg])
    assert float((R[exact] - Rf[exact]).abs().max()) == 0.0 and float((R[bwd] - Rf[bwd]).abs().max()) < 1e-15
    assert bool(((dx[bwd] - dxf[bwd]).abs() <= 1e-12 * dx[bwd].abs()).all())
    # the fp32 evaluation of the same formula is within the bound the kernel is held to on these rows (1e-5 of the float64 value per entry)
    R32, dx32 = H.rot6d_formula(x, g, torch.float32)
    assert bool(((dx32[bwd].double() - dx[bwd]).abs() <= 1e-5 * dx[bwd].abs()).all()) and float((R32[exact].double() - R[exact]).abs().max()) == 0.0
    assert float((R32[bwd].double() - R[bwd]).abs().max()) <= 2e-6
    for i, (kind, row, e) in enumerate(deg):
        if kind == 'a1=0':
            a2 = row.double()[1::2]
            assert bool((R[i][:, 0] == 0).all()) and bool((R[i][:, 2] == 0).all()) and float((R[i][:, 1] - a2 / a2.norm()).abs().max()) < 1e-15
            assert float(dx[i].abs().max()) > 1e10                # d b1 / d a1 = 1 / 1e-12 in the clamped branch
        if kind == 'a2=0':
            assert bool((R[i][:, 1] == 0).all()) and bool((R[i][:, 2] == 0).all())
        if kind == 'tiny-u':                                      # the clamped quotient is not zero: the projected branch would differ by a quarter
            b2 = R[i][:, 1]
            assert 0.2 < float(b2.norm()) < 0.6 and float(dx[i].abs().max()) > 1e10
            gu_clamped = dx[i][1::2]                              # d a2 = gu - (gu.b1) b1
            assert float(gu_clamped.abs().max()) > 1e10
        if kind == 'tiny-a1':
            assert 0.2 < float(R[i][:, 0].norm()) < 0.6 and float(dx[i][0::2].abs().max()) > 1e10
        if kind == 'collinear' and e is True:
            assert bool((R[i][:, 1] == 0).all()) and bool((R[i][:, 2] == 0).all()) and float(dx[i].abs().max()) > 1e10


def test_projection_references_against_the_oracle_and_fp32_measurements():
    for B, N, ld in H.ORTHO:
        pts, cam = H.det((B, N, 3), 500), H.cam_rows(B, ld, 501)
        want = H.ortho_reference(pts, cam)
        ora = O.orthographic_project(pts.double(), cam[:, :3].double())
        assert float(((want.double() - ora).abs() / ora.abs().clamp_min(1e-30)).max()) <= 2.0 ** -23 + 2.0 ** -46
    for N in H.ORTHO_BWD_N:
        for B in H.ORTHO_BWD_B:
            pts, cam, dout = H.det((B, N, 3), 510), H.cam_rows(B, 3, 511), H.det((B, N, 2), 512)
            dp, dcam, bound = H.ortho_bwd_reference(pts, cam, dout)
            p64, c64 = pts.double().requires_grad_(), cam.double().requires_grad_()
            O.orthographic_project(p64, c64).backward(dout.double())
            assert float((dcam - c64.grad).abs().max()) <= 1e-12 * max(1.0, float(dcam.abs().max()))
            assert float((dp.double() - p64.grad).abs().max()) <= 2.0 ** -23 and bool((dp[:, :, 2] == 0).all())
    e = H.persp_fp32_cpu_error()
    t = H.targets_fp32_cpu_error()
    print('MEASURED perspective_project fp32 CPU evaluation: %.3e (the kernel gets 4x: %.3e); project_targets: %.3e (4x: %.3e)' % (e, 4 * e, t, 4 * t))
    assert 0 < e < 0.05 and 0 < t < 0.05                   # (pixels, at coordinates of a few thousand)
    for B, N in H.PERSP:
        pts, rot, tr, K = H.persp_inputs(B, N, 1)
        assert bool((K[:, 0, 1] != 0).all()) and float(tr[:, 2].min()) >= 2.0
        p = pts.double() @ rot.double().transpose(1, 2) + tr.double()[:, None]
        p = p / p[:, :, 2:]
        want = (p @ K.double().transpose(1, 2))[:, :, :2]
        assert float((want - H.persp_eval(pts, rot, tr, K, torch.float64)).abs().max()) < 1e-9
    assert H.COCO == [24, 26, 25, 28, 27, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8] and H.H36M14 == [79, 78, 77, 74, 75, 76, 89, 88, 87, 84, 85, 86, 81, 83]


def test_rodrigues_fp32_measurement():
    for n in (257,):
        aa, fam = H.rodrigues_rows(n)
        keep = ~H.rodrigues_excluded(aa)
        e = (O.batch_rodrigues(aa).double() - O.batch_rodrigues(aa.double())).abs().amax((1, 2))
        for f in sorted(set(fam)):
            sel = torch.tensor([x == f for x in fam]) & keep
            if bool(sel.any()):
                print('MEASURED rodrigues fp32 CPU evaluation, %s rows: %.2e' % (f, float(e[sel].max())))
        assert float(e[torch.tensor([x == 'random' for x in fam])].max()) < 2e-6
    assert bool(torch.equal(O.batch_rodrigues(torch.zeros(1, 3).double())[0], torch.eye(3, dtype=torch.float64)))


def test_adam_reference_against_torch_optim():
    for step in H.ADAM_STEPS:
        p, g, m, v = H.adam_data(257, step)
        ref = H.adam_reference(p, g, m, v, step, 1.0)
        q = torch.nn.Parameter(p.double().clone())
        opt = torch.optim.Adam([q], lr=H.f32(H.ADAM_LR), betas=(H.f32(H.ADAM_B1), H.f32(H.ADAM_B2)), eps=H.f32(H.ADAM_EPS))
        q.grad = g.double().clone()
        if step > 1:
            opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.double().clone(), exp_avg_sq=v.double().clone())
        opt.step()
        st = opt.state[q]
        assert float((st['exp_avg'] - ref['m']).abs().max()) <= 1e-15 * max(1.0, float(ref['m'].abs().max()))
        assert float(((st['exp_avg_sq'] - ref['v']).abs() / ref['v'].clamp_min(1e-300)).max()) <= 1e-12
        assert float((q.detach() - ref['p']).abs().max()) <= 1e-15
        # an fp32 evaluation on the CPU (no contraction) meets the bounds the kernel is held to
        for gs in H.ADAM_GRAD_SCALES:
            r = H.adam_reference(p, g, m, v, step, gs)
            b1, b2 = torch.tensor(H.ADAM_B1), torch.tensor(H.ADAM_B2)
            gi = g * torch.tensor(gs, dtype=torch.float32)
            mi = b1 * m + (1 - b1) * gi
            vi = b2 * v + (1 - b2) * gi * gi
            ss = torch.tensor(H.f32(H.ADAM_LR) / (1 - H.f32(H.ADAM_B1) ** step), dtype=torch.float32)
            ic = torch.tensor(1 / (1 - H.f32(H.ADAM_B2) ** step) ** 0.5, dtype=torch.float32)
            pi = p - ss * mi / (vi.sqrt() * ic + torch.tensor(H.ADAM_EPS))
            normal = r['v'] >= 2.0 ** -126
            assert bool(((mi.double() - r['m']).abs() <= r['m_bound']).all()) and bool(((vi.double() - r['v']).abs() <= r['v_bound'])[normal].all())
            assert bool(((pi.double() - r['p']).abs() <= r['p_bound']).all()) and bool(torch.equal(pi[r['untouched']], p[r['untouched']]))


def test_mse_reference_against_mse_loss():
    for rows, cols in [(3, 34), (70, 216), (4681, 14)]:
        for mk in H.MSE_MASKS:
            for sc in H.MSE_SCALES:
                pred, tgt, mask = H.mse_data(rows, cols, mk, sc)
                r = H.mse_reference(pred, tgt, mask, sc)
                idx = torch.arange(rows) if mask is None else mask.nonzero().flatten()
                t64 = tgt.double() * H.f32(sc[0]) + H.f32(sc[1])
                want = F.mse_loss(pred.double()[idx], t64[idx])
                assert abs(r['mean'] - float(want)) <= 1e-12 * float(want) and r['count'] == idx.numel() * cols
                assert abs(r['sum'] - float(F.mse_loss(pred.double()[idx], t64[idx], reduction='sum'))) <= 1e-12 * r['sum']
    pred, tgt, mask = H.mse_data(7, 10, 'none', H.MSE_SCALES[0])
    r = H.mse_reference(pred, tgt, mask, H.MSE_SCALES[0])
    assert r['sum'] == 0.0 and r['count'] == 0 and r['mean'] != r['mean']
    assert bool(torch.isnan(F.mse_loss(pred[:0], tgt[:0])))                   # a mean over nothing is NaN in the reference too


# ------------------------------------------------------------------------------------------------------------------------------------ argument checks

def _err(lib):
    return lib.straps_last_error().decode()


def test_linear_fwd_argument_checks(lib):
    """kdim % 8, ldx % 4, ldw % 4, ldx < kdim and a misaligned x or w each return the error code with the entry point's name in straps_last_error
    (all of them return before a launch: the addresses are never dereferenced)"""
    a = 0x7f0000001000                    # a 16-byte aligned address nobody reads
    p = C.c_void_p
    good = dict(x=a, ldx=16, w=a, ldw=16, m=2, n=3, k=16)
    for change in (dict(k=12, ldx=12, ldw=12), dict(ldx=18), dict(ldw=18), dict(ldx=12), dict(ldw=12), dict(x=a + 4), dict(w=a + 8), dict(x=0), dict(k=0)):
        c = dict(good, **change)
        rc = lib.straps_linear_fwd(p(c['x']), c['ldx'], p(c['w']), c['ldw'], None, None, p(a), c['n'], c['m'], c['n'], c['k'], 0, None)
        assert rc != 0 and 'straps_linear_fwd' in _err(lib), change


def test_gemm_multi_and_projection_argument_checks(lib):
    a = 0x7f0000001000
    ok = hipabi.gemm_desc(a, 4, 1, a, 4, 1, a, 4, 2, 2, 4)
    arr1 = (hipabi.GemmDesc * 9)(*([ok] * 9))
    assert lib.straps_gemm_multi(arr1, 0, None) != 0 and 'straps_gemm_multi' in _err(lib)
    assert lib.straps_gemm_multi(arr1, 9, None) != 0 and 'straps_gemm_multi' in _err(lib)
    for bad in (hipabi.gemm_desc(a, 4, 1, a, 4, 1, None, 4, 2, 2, 4), hipabi.gemm_desc(a, 4, 1, a, 4, 1, a, 4, 2, 2, 0)):
        for pos in (0, 1):
            descs = [ok, ok]
            descs[pos] = bad
            assert lib.straps_gemm_multi((hipabi.GemmDesc * 2)(*descs), 2, None) != 0 and 'straps_gemm_multi: problem %d' % pos in _err(lib)
    p = C.c_void_p
    assert lib.straps_orthographic_project_bwd(p(a), p(a), 3, p(a), None, None, 1, 1, None) != 0 and 'straps_orthographic_project_bwd' in _err(lib)
