// regressor.hip -- the whole eval-mode regressor forward behind one C entry point (straps_regressor_*, include/straps_hip.h).
//
// Host scheduling only: every launch below is an existing entry point of this library, called with the arguments
// SingleInputRegressor.eval() passes to it from Python (encoder_exec.py / ief_module.py), so the results are bit-identical to the
// module's.  The network (regressor_net.h) is walked once per call into a Plan that adds the offsets of the prepared buffer; a Work
// gives the workspace slots for one input.
#include "regressor_net.h"

namespace {

struct Plan : Net {
    // prepared buffer (bytes)
    size_t ss[kMaxConvs];           // folded scale [cout] then shift [cout], per convolution
    size_t wk[kMaxConvs];           // fp32 route: KRSC weights, per convolution
    size_t stem_w, stem_ss, table, planes, w1f, w1e, w3, fc1b, fc2w, fc2b, fc3b, init, prepared_bytes;
};

void make_plan(const straps_regressor_desc_t* d, Plan& p) {
    make_net(d, p);
    size_t b = 0;
    auto take = [&](size_t bytes) { const size_t o = b; b = align_up(b + bytes); return o; };
    p.stem_w = take(straps_stem_weight_floats(p.cin) * sizeof(float));
    p.stem_ss = take(2 * 64 * sizeof(float));
    for (int i = 0; i < p.nconvs; ++i) p.ss[i] = take(2 * (size_t)p.convs[i].cout * sizeof(float));
    p.table = p.planes = 0;
    if (p.precision == 0) {
        p.table = take((size_t)p.nconvs * sizeof(straps_pack_desc_t));
        p.planes = take(3 * (size_t)p.ps * sizeof(unsigned short));
    } else if (p.precision == 3) {      // bf16: one plane, every layer at its `first` (multiples of 64 x 64 elements: 16-byte aligned)
        p.planes = take((size_t)p.ps * sizeof(unsigned short));
    } else {
        for (int i = 0; i < p.nconvs; ++i) p.wk[i] = take((size_t)p.convs[i].weights() * sizeof(float));
    }
    p.w1f = take((size_t)p.H1 * p.F * sizeof(float));
    p.w1e = take((size_t)p.H1 * kEstLd * sizeof(float));
    p.w3 = take((size_t)((kNumParams + 31) / 32 * 32) * p.H2 * sizeof(float));
    p.fc1b = take(p.H1 * sizeof(float));
    p.fc2w = take((size_t)p.H2 * p.H1 * sizeof(float));
    p.fc2b = take(p.H2 * sizeof(float));
    p.fc3b = take(kNumParams * sizeof(float));
    p.init = take(kNumParams * sizeof(float));
    p.prepared_bytes = b;
}

// Workspace slots for one (B, H, W).  Between the stem and the pooled input only the stem output lives; afterwards a fixed set of
// slots is reused by every residual unit:
//   io[0], io[1] : unit inputs / outputs (ping-pong), fp32 + (bf16x3) their planes / (bf16) their plane -- io[0] first holds the pooled stem output
//   idt          : fp32 output of a unit's projection (the identity of units with a downsample)
//   mid[0..1]    : outputs of a unit's inner convolutions (bf16x3 / bf16: planes only, nothing reads their fp32 form; fp32: fp32)
//   ief          : features, fc1 feature half, the iterations' estimates [T + 1][B][160], one hidden pair [B][H1], [B][H2]
// The stem output overlaps everything behind io[0]: it is dead once the max pool has written io[0].
struct Work {
    Geometry g;
    long long io_ps, mid_ps[2];
    size_t nzmask, io[2], io_planes[2], idt, mid[2], stem_out;
    size_t feat, c1, ests, h1, h2, bytes;
};

bool make_work(const Plan& p, int B, int H, int W, Work& w) {
    if (!make_geometry(p, B, H, W, w.g)) return false;
    const int npl = p.precision == 0 ? 3 : p.precision == 3 ? 1 : 0;      // activation planes
    long long io = (long long)B * w.g.Hp * w.g.Wp * 64, idt = 0, mid[2] = {0, 0};
    auto grow = [&](long long& slot, int i) {
        const long long n = (long long)B * w.g.e[i].Ho * w.g.e[i].Wo * p.convs[i].cout;
        slot = n > slot ? n : slot;
    };
    for (int ui = 0; ui < p.nunits; ++ui) {
        const Unit& u = p.units[ui];
        if (u.has_ds) grow(idt, u.ds);
        for (int ci = 0; ci < u.nconv; ++ci) grow(ci == u.nconv - 1 ? io : mid[ci], u.c[ci]);
    }
    w.io_ps = round8(io);
    for (int i = 0; i < 2; ++i) w.mid_ps[i] = round8(mid[i]);
    size_t b = 0;
    auto take = [&](size_t bytes) { const size_t o = b; b = align_up(b + bytes); return o; };
    w.nzmask = take(straps_stem_nzmask_words(B, p.cin, H, W) * sizeof(uint32_t));
    w.io[0] = take(io * sizeof(float));
    w.io_planes[0] = npl ? take(npl * (size_t)w.io_ps * sizeof(unsigned short)) : 0;
    const size_t tail = b;
    w.io[1] = take(io * sizeof(float));
    w.io_planes[1] = npl ? take(npl * (size_t)w.io_ps * sizeof(unsigned short)) : 0;
    w.idt = take((idt ? idt : 1) * sizeof(float));
    for (int i = 0; i < 2; ++i) {
        const size_t n = mid[i] ? (size_t)mid[i] : 1;
        w.mid[i] = npl ? take(npl * (size_t)round8(n) * sizeof(unsigned short)) : take(n * sizeof(float));
    }
    w.feat = take((size_t)B * p.F * sizeof(float));
    w.c1 = take((size_t)B * p.H1 * sizeof(float));
    w.ests = take((size_t)(p.iters + 1) * B * kEstLd * sizeof(float));
    w.h1 = take((size_t)B * p.H1 * sizeof(float));
    w.h2 = take((size_t)B * p.H2 * sizeof(float));
    w.stem_out = tail;
    const size_t stem_end = align_up(tail + (size_t)B * w.g.Hs * w.g.Ws * 64 * sizeof(float));
    w.bytes = b > stem_end ? b : stem_end;
    return true;
}

#define RG_HIP(expr, what)                                                                          \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess) {                                                                    \
            straps_set_error("straps_regressor_prepare: %s failed: %s", what, hipGetErrorString(e__)); \
            return STRAPS_EHIP;                                                                     \
        }                                                                                           \
    } while (0)

}  // namespace

extern "C" size_t straps_regressor_param_floats(const straps_regressor_desc_t* d) {
    if (check_desc(d, false)) return 0;
    Net n;
    make_net(d, n);
    return (size_t)n.inf_floats;
}

extern "C" size_t straps_regressor_prepared_bytes(const straps_regressor_desc_t* d) {
    if (check_desc(d, false)) return 0;
    Plan p;
    make_plan(d, p);
    return p.prepared_bytes;
}

extern "C" size_t straps_regressor_workspace_bytes(const straps_regressor_desc_t* d, int batch, int h, int w) {
    if (check_desc(d, false)) return 0;
    Plan p;
    make_plan(d, p);
    Work wk;
    if (!make_work(p, batch, h, w, wk)) return 0;
    return wk.bytes;
}

extern "C" int straps_regressor_prepare(const straps_regressor_desc_t* d, const float* params, void* prepared, void* stream) {
    const char* bad = check_desc(d, false);
    STRAPS_REQUIRE(!bad, "straps_regressor_prepare: %s", bad);
    STRAPS_REQUIRE(params, "straps_regressor_prepare: null pointer `params`");
    STRAPS_REQUIRE(prepared, "straps_regressor_prepare: null pointer `prepared`");
    STRAPS_REQUIRE(((uintptr_t)params & 15) == 0, "straps_regressor_prepare: `params` must be 16-byte aligned");
    STRAPS_REQUIRE(((uintptr_t)prepared & (kAlign - 1)) == 0, "straps_regressor_prepare: `prepared` must be %zu-byte aligned", kAlign);
    Plan p;
    make_plan(d, p);
    hipStream_t st = (hipStream_t)stream;
    char* pb = (char*)prepared;
    auto f = [&](size_t off) { return (float*)(pb + off); };
    auto bn_fold = [&](const Conv& cv, size_t ss_off) {
        const float* g = params + cv.inf_bn;
        const int c = cv.cout;
        return straps_bn_fold(g, g + c, g + 2 * c, g + 3 * c, kBnEps, f(ss_off), f(ss_off) + c, c, stream);
    };
    // stem: fragment-order weights and its folded BatchNorm
    RG_CALL(straps_pack_stem_weight(params + p.stem.inf_w, f(p.stem_w), p.cin, stream));
    RG_CALL(bn_fold(p.stem, p.stem_ss));
    for (int i = 0; i < p.nconvs; ++i) RG_CALL(bn_fold(p.convs[i], p.ss[i]));
    if (p.precision == 0) {
        // every layer's bf16x3 forward planes in one launch (ResNet.prepack without the data-gradient layout)
        straps_pack_desc_t table[kMaxConvs];
        for (int i = 0; i < p.nconvs; ++i) {
            const Conv& cv = p.convs[i];
            table[i].src = params + cv.inf_w;
            table[i].dst_krsc = nullptr;
            table[i].dst_crsk = nullptr;
            table[i].o = cv.cout; table[i].c = cv.cin; table[i].r = cv.k; table[i].s = cv.k;
            table[i].first = cv.first;
        }
        RG_HIP(hipMemcpyAsync(pb + p.table, table, p.nconvs * sizeof(straps_pack_desc_t), hipMemcpyHostToDevice, st), "hipMemcpyAsync(descriptor table)");
        RG_CALL(straps_pack_conv_weights_batched_x3((const straps_pack_desc_t*)(pb + p.table), p.nconvs, p.conv_total,
                                                    (unsigned short*)(pb + p.planes), nullptr, p.ps, stream));
        // (the descriptor table lives in this frame: it must have reached the device before the function returns)
        RG_HIP(hipStreamSynchronize(st), "hipStreamSynchronize");
    } else if (p.precision == 3) {
        // bf16: every layer's forward weights as one rn_bf16 plane (ResNet._packed_weight_bf16)
        for (int i = 0; i < p.nconvs; ++i) {
            const Conv& cv = p.convs[i];
            RG_CALL(straps_pack_conv_weight_bf16(params + cv.inf_w, (unsigned short*)(pb + p.planes) + cv.first, cv.cout, cv.cin, cv.k, cv.k, stream));
        }
    } else {
        for (int i = 0; i < p.nconvs; ++i) {
            const Conv& cv = p.convs[i];
            RG_CALL(straps_pack_conv_weight(params + cv.inf_w, f(p.wk[i]), cv.cout, cv.cin, cv.k, cv.k, stream));
        }
    }
    // IEF: the repacked fc1 / fc3 views, and copies of everything else the iterations read (the forward never touches `params`)
    const Ief& l = p.ief_inf;
    RG_CALL(straps_ief_pack(params + l.fc1w, params + l.fc3w, f(p.w1f), f(p.w1e), f(p.w3), p.F, kNumParams, p.H1, p.H2, kEstLd, stream));
    const struct { size_t dst; long long src, n; } copies[] = {
        {p.fc1b, l.fc1b, p.H1}, {p.fc2w, l.fc2w, (long long)p.H2 * p.H1}, {p.fc2b, l.fc2b, p.H2},
        {p.fc3b, l.fc3b, kNumParams}, {p.init, p.inf_init, kNumParams}};
    for (const auto& c : copies)
        RG_HIP(hipMemcpyAsync(f(c.dst), params + c.src, c.n * sizeof(float), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(IEF parameters)");
    RG_HIP(hipStreamSynchronize(st), "hipStreamSynchronize");
    return STRAPS_OK;
}

extern "C" int straps_regressor_fwd_infer(const straps_regressor_desc_t* d, const void* prepared, const float* x, int batch, int h, int w,
                                          float* est, int ld_est, float* rotmats, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* fn = "straps_regressor_fwd_infer";
    RG_CALL(check_args(fn, d, false, x, batch, h, w, workspace));
    STRAPS_REQUIRE(prepared, "%s: null pointer `prepared`", fn);
    STRAPS_REQUIRE(est, "%s: null pointer `est`", fn);
    STRAPS_REQUIRE(ld_est >= kNumParams, "%s: `ld_est` must be >= %d (got %d)", fn, kNumParams, ld_est);
    STRAPS_REQUIRE(((uintptr_t)prepared & (kAlign - 1)) == 0, "%s: `prepared` must be %zu-byte aligned", fn, kAlign);
    STRAPS_REQUIRE(((uintptr_t)est & 3) == 0 && ((uintptr_t)rotmats & 3) == 0, "%s: `est` and `rotmats` must be float-aligned", fn);
    Plan p;
    make_plan(d, p);
    Work wk;
    STRAPS_REQUIRE(make_work(p, batch, h, w, wk), "%s: input %d x %d is too small for resnet%d", fn, h, w, p.layers);
    STRAPS_REQUIRE(workspace_bytes >= wk.bytes, "%s: `workspace_bytes` is %zu, this batch needs %zu (straps_regressor_workspace_bytes)", fn,
                   workspace_bytes, wk.bytes);
    const bool x3 = p.precision == 0, b16 = p.precision == 3;
    const char* pb = (const char*)prepared;
    char* ws = (char*)workspace;
    auto pf = [&](size_t off) { return (const float*)(pb + off); };
    auto wf = [&](size_t off) { return (float*)(ws + off); };
    auto wp = [&](size_t off) { return (unsigned short*)(ws + off); };
    const unsigned short* wplanes = (const unsigned short*)(pb + p.planes);
    const int B = batch, C = p.cin;
    const Geometry& g = wk.g;

    // ---- stem: non-zero map, conv 7x7/s2 with folded BatchNorm + ReLU (encoder_forward, eval), max pool into io[0] ----
    uint32_t* nz = (uint32_t*)(ws + wk.nzmask);
    RG_CALL(straps_stem_nzmask(x, nz, B, C, h, w, stream));
    RG_CALL(straps_stem_fwd(x, pf(p.stem_w), pf(p.stem_ss), pf(p.stem_ss) + 64, 1, wf(wk.stem_out), nullptr, nz, B, C, h, w, stream));
    RG_CALL(straps_maxpool_fwd(wf(wk.stem_out), wf(wk.io[0]), B, g.Hs, g.Ws, 64, stream));
    int cur = 0;
    if (x3)      // the pooled input is the only activation split into planes by a pass of its own
        RG_CALL(straps_split3_bf16_cm(wf(wk.io[0]), wp(wk.io_planes[0]), (long long)B * g.Hp * g.Wp, 64, wk.io_ps, stream));
    if (b16)
        RG_CALL(straps_split_bf16_cm(wf(wk.io[0]), wp(wk.io_planes[0]), (long long)B * g.Hp * g.Wp, 64, stream));

    // ---- residual stages (encoder_exec._residual_stages, eval without a tape) ----
    for (int ui = 0; ui < p.nunits; ++ui) {
        const Unit& u = p.units[ui];
        const float* in = wf(wk.io[cur]);
        const unsigned short* in3 = (x3 || b16) ? wp(wk.io_planes[cur]) : nullptr;
        const float* idt = in;
        if (u.has_ds) {     // projection: no ReLU, fp32 output only
            const Conv& cv = p.convs[u.ds];
            const Extent& e = g.e[u.ds];
            const float* ss = pf(p.ss[u.ds]);
            if (x3)
                RG_CALL(straps_conv_fwd_x3(in3, wk.io_ps, wplanes + cv.first, p.ps, ss, ss + cv.cout, nullptr, 0, wf(wk.idt), nullptr,
                                           B, e.H, e.W, cv.cin, cv.cout, 1, 1, cv.stride, 0, 0, stream));
            else if (b16)
                RG_CALL(straps_conv_fwd_bf16(in3, wplanes + cv.first, ss, ss + cv.cout, nullptr, 0, wf(wk.idt), nullptr, B, e.H, e.W, cv.cin, cv.cout, 1, 1,
                                             cv.stride, 0, 0, stream));
            else
                RG_CALL(straps_conv_fwd(in, pf(p.wk[u.ds]), ss, ss + cv.cout, nullptr, 0, wf(wk.idt), nullptr, B, e.H, e.W, cv.cin, cv.cout, 1, 1,
                                        cv.stride, 0, 0, stream));
            idt = wf(wk.idt);
        }
        const float* t = in;
        const unsigned short* t3 = in3;
        long long t_ps = wk.io_ps;
        for (int ci = 0; ci < u.nconv; ++ci) {
            const int i = u.c[ci];
            const Conv& cv = p.convs[i];
            const Extent& e = g.e[i];
            const float* ss = pf(p.ss[i]);
            const float* res = cv.last ? idt : nullptr;
            float* y = cv.last ? wf(wk.io[cur ^ 1]) : ((x3 || b16) ? nullptr : wf(wk.mid[ci]));
            unsigned short* y3 = (x3 || b16) ? (cv.last ? wp(wk.io_planes[cur ^ 1]) : wp(wk.mid[ci])) : nullptr;
            const long long y_ps = cv.last ? wk.io_ps : wk.mid_ps[ci];
            if (x3)      // ReLU outputs write their planes in the epilogue; the fp32 tensor only for a unit's output
                RG_CALL(straps_conv_fwd_x3p(t3, t_ps, wplanes + cv.first, p.ps, ss, ss + cv.cout, res, 1, y, y3, y_ps,
                                            B, e.H, e.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0, stream));
            else if (b16)      // the same with one plane
                RG_CALL(straps_conv_fwd_bf16(t3, wplanes + cv.first, ss, ss + cv.cout, res, 1, y, y3, B, e.H, e.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride,
                                             cv.pad, 0, stream));
            else
                RG_CALL(straps_conv_fwd(t, pf(p.wk[i]), ss, ss + cv.cout, res, 1, y, nullptr, B, e.H, e.W, cv.cin, cv.cout, cv.k, cv.k,
                                        cv.stride, cv.pad, 0, stream));
            t = y;
            t3 = y3;
            t_ps = y_ps;
        }
        cur ^= 1;
    }

    // ---- global average pool, then the IEF iterations with one hidden pair ----
    RG_CALL(ief_forward(p, B, wf(wk.io[cur]), g.Hf * g.Wf, pf(p.init), pf(p.w1f), pf(p.w1e), pf(p.fc1b), pf(p.fc2w), pf(p.fc2b), pf(p.w3),
                        pf(p.fc3b), wf(wk.feat), wf(wk.c1), wf(wk.ests), wf(wk.h1), 0, wf(wk.h2), 0, est, ld_est, stream));
    if (rotmats) RG_CALL(straps_rot6d_fwd(est + 3, ld_est, 24, rotmats, B, stream));
    return STRAPS_OK;
}
