// regressor.hip -- the whole eval-mode regressor forward behind one C entry point (straps_regressor_*, include/straps_hip.h).
//
// Host scheduling only: every launch below is an existing entry point of this library, called with the arguments
// SingleInputRegressor.eval() passes to it from Python (encoder_exec.py / ief_module.py), so the results are bit-identical to the
// module's.  The network geometry is walked once per call into a Plan that gives the offsets of the flat parameter buffer, of the
// prepared buffer and of the workspace slots.
#include "common.h"

namespace {

constexpr int kEstLd = 160;           // IEF estimate row stride (ief_module.EST_LD): 157 padded to a multiple of 8
constexpr int kNumParams = 157;       // cam 3 | pose 24 x 6 | shape 10
constexpr float kBnEps = 1e-5f;       // nn.BatchNorm2d's default eps (not part of the state dict)
constexpr size_t kAlign = 256;        // every region of the prepared buffer and the workspace starts on this boundary
constexpr int kMaxConvs = 64;         // resnet50 has 52 convolutions besides the stem

size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }
long long round8(long long v) { return (v + 7) / 8 * 8; }
int conv_out(int h, int k, int s, int p) { return (h + 2 * p - k) / s + 1; }

struct Conv {
    int cin, cout, k, stride, pad;
    long long w_off;       // params: OIHW weight (floats)
    long long bn_off;      // params: gamma, beta, running_mean, running_var (cout floats each)
    long long first;       // element offset of this layer in the packed weights (state-dict order)
    size_t ss_off;         // prepared: folded scale [cout] then shift [cout]
    size_t wk_off;         // prepared, fp32 route: KRSC weights
};

struct Unit {
    Conv c[3];
    int nconv;
    bool has_ds;
    Conv ds;
};

struct Plan {
    int layers, cin, iters, precision;
    int F, H1, H2;
    long long stem_w_off, stem_bn_off;
    Unit units[16];
    int nunits;
    Conv* convs[kMaxConvs];         // non-stem convolutions in state-dict order (= ResNet.prepack's order)
    int nconvs;
    long long conv_total;           // sum of the non-stem weight elements
    long long fc1w_off, fc1b_off, fc2w_off, fc2b_off, fc3w_off, fc3b_off, init_off, param_floats;
    // prepared buffer (bytes)
    size_t stem_w, stem_ss, table, planes, w1f, w1e, w3, fc1b, fc2w, fc2b, fc3b, init, prepared_bytes;
    long long ps;                   // plane stride of the bf16x3 weight planes (bf16: the element count of the one plane, rounded up to 8)
};

// nullptr + text when the description is invalid (the text names the field)
const char* check_desc(const straps_regressor_desc_t* d) {
    if (!d) return "null pointer `desc`";
    if (d->layers != 18 && d->layers != 50) return "`layers` must be 18 or 50";
    // (the stem keeps all input channels' weights in LDS: 256 channels fit its 160 KiB)
    if (d->in_channels < 1 || d->in_channels > 256) return "`in_channels` must be in [1, 256]";
    if (d->ief_iters < 1 || d->ief_iters > 64) return "`ief_iters` must be in [1, 64]";
    // (2 is unassigned: it stays invalid)
    if (d->precision != 0 && d->precision != 1 && d->precision != 3) return "`precision` must be 0 (bf16x3), 1 (fp32) or 3 (bf16)";
    return nullptr;
}

void make_plan(const straps_regressor_desc_t* d, Plan& p) {
    p.layers = d->layers;
    p.cin = d->in_channels;
    p.iters = d->ief_iters;
    p.precision = d->precision;
    const bool bottleneck = d->layers == 50;
    const int blocks18[4] = {2, 2, 2, 2}, blocks50[4] = {3, 4, 6, 3};
    const int* blocks = bottleneck ? blocks50 : blocks18;
    const int expansion = bottleneck ? 4 : 1;
    long long off = 0, first = 0;
    auto bn = [&](int c) { const long long o = off; off += 4LL * c; return o; };
    auto conv = [&](Conv& cv, int cin, int cout, int k, int stride, int pad) {
        cv.cin = cin; cv.cout = cout; cv.k = k; cv.stride = stride; cv.pad = pad;
        cv.w_off = off;
        off += (long long)cout * cin * k * k;
        cv.bn_off = bn(cout);
        cv.first = first;
        first += (long long)cout * cin * k * k;
        p.convs[p.nconvs++] = &cv;
    };
    p.nconvs = 0;
    p.nunits = 0;
    p.stem_w_off = off;
    off += 64LL * p.cin * 49;
    p.stem_bn_off = bn(64);
    int inplanes = 64;
    for (int li = 0; li < 4; ++li) {
        const int planes = 64 << li, stride = li == 0 ? 1 : 2;
        for (int bi = 0; bi < blocks[li]; ++bi) {
            Unit& u = p.units[p.nunits++];
            const int s = bi == 0 ? stride : 1, outp = planes * expansion;
            // state-dict order of a unit: its own convolutions, then the projection (ResidualUnit registers `downsample` last)
            if (bottleneck) {
                u.nconv = 3;
                conv(u.c[0], inplanes, planes, 1, 1, 0);
                conv(u.c[1], planes, planes, 3, s, 1);
                conv(u.c[2], planes, outp, 1, 1, 0);
            } else {
                u.nconv = 2;
                conv(u.c[0], inplanes, planes, 3, s, 1);
                conv(u.c[1], planes, planes, 3, 1, 1);
            }
            u.has_ds = bi == 0 && (s != 1 || inplanes != outp);
            if (u.has_ds) conv(u.ds, inplanes, outp, 1, s, 0);
            inplanes = outp;
        }
    }
    p.conv_total = first;
    p.F = inplanes;
    p.H1 = p.H2 = bottleneck ? 1024 : 512;
    p.fc1w_off = off; off += (long long)p.H1 * (p.F + kNumParams);
    p.fc1b_off = off; off += p.H1;
    p.fc2w_off = off; off += (long long)p.H2 * p.H1;
    p.fc2b_off = off; off += p.H2;
    p.fc3w_off = off; off += (long long)kNumParams * p.H2;
    p.fc3b_off = off; off += kNumParams;
    p.init_off = off; off += kNumParams;
    p.param_floats = off;

    size_t b = 0;
    auto take = [&](size_t bytes) { const size_t o = b; b = align_up(b + bytes); return o; };
    p.stem_w = take(straps_stem_weight_floats(p.cin) * sizeof(float));
    p.stem_ss = take(2 * 64 * sizeof(float));
    for (int i = 0; i < p.nconvs; ++i) p.convs[i]->ss_off = take(2 * (size_t)p.convs[i]->cout * sizeof(float));
    p.ps = round8(p.conv_total);
    p.table = p.planes = 0;
    if (p.precision == 0) {
        p.table = take((size_t)p.nconvs * sizeof(straps_pack_desc_t));
        p.planes = take(3 * (size_t)p.ps * sizeof(unsigned short));
    } else if (p.precision == 3) {      // bf16: one plane, every layer at its `first` (multiples of 64 x 64 elements: 16-byte aligned)
        p.planes = take((size_t)p.ps * sizeof(unsigned short));
    } else {
        for (int i = 0; i < p.nconvs; ++i) {
            Conv& cv = *p.convs[i];
            cv.wk_off = take((size_t)cv.cout * cv.cin * cv.k * cv.k * sizeof(float));
        }
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
    int Hs, Ws, Hp, Wp;                     // stem output, pooled
    long long io_elems, io_ps, idt_elems, mid_elems[2], mid_ps[2];
    size_t nzmask, io[2], io_planes[2], idt, mid[2], stem_out;
    size_t feat, c1, ests, h1, h2, bytes;
};

bool make_work(const Plan& p, int B, int H, int W, Work& w) {
    if (B <= 0 || H < 7 || W < 7) return false;
    const int npl = p.precision == 0 ? 3 : p.precision == 3 ? 1 : 0;      // activation planes
    w.Hs = conv_out(H, 7, 2, 3); w.Ws = conv_out(W, 7, 2, 3);
    w.Hp = conv_out(w.Hs, 3, 2, 1); w.Wp = conv_out(w.Ws, 3, 2, 1);
    long long io = (long long)B * w.Hp * w.Wp * 64, idt = 0, mid[2] = {0, 0};
    int h = w.Hp, wd = w.Wp;
    for (int ui = 0; ui < p.nunits; ++ui) {
        const Unit& u = p.units[ui];
        if (u.has_ds) {
            const long long n = (long long)B * conv_out(h, 1, u.ds.stride, 0) * conv_out(wd, 1, u.ds.stride, 0) * u.ds.cout;
            idt = n > idt ? n : idt;
        }
        for (int ci = 0; ci < u.nconv; ++ci) {
            const Conv& cv = u.c[ci];
            h = conv_out(h, cv.k, cv.stride, cv.pad);
            wd = conv_out(wd, cv.k, cv.stride, cv.pad);
            if (h <= 0 || wd <= 0) return false;
            const long long n = (long long)B * h * wd * cv.cout;
            long long& slot = ci == u.nconv - 1 ? io : mid[ci];
            slot = n > slot ? n : slot;
        }
    }
    w.io_elems = io;
    w.io_ps = round8(io);
    w.idt_elems = idt;
    for (int i = 0; i < 2; ++i) { w.mid_elems[i] = mid[i]; w.mid_ps[i] = round8(mid[i]); }
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
    const size_t stem_end = align_up(tail + (size_t)B * w.Hs * w.Ws * 64 * sizeof(float));
    w.bytes = b > stem_end ? b : stem_end;
    return true;
}

#define RG_CALL(expr)                         \
    do {                                      \
        const int rc__ = (expr);              \
        if (rc__ != STRAPS_OK) return rc__;   \
    } while (0)

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
    if (check_desc(d)) return 0;
    Plan p;
    make_plan(d, p);
    return (size_t)p.param_floats;
}

extern "C" size_t straps_regressor_prepared_bytes(const straps_regressor_desc_t* d) {
    if (check_desc(d)) return 0;
    Plan p;
    make_plan(d, p);
    return p.prepared_bytes;
}

extern "C" size_t straps_regressor_workspace_bytes(const straps_regressor_desc_t* d, int batch, int h, int w) {
    if (check_desc(d)) return 0;
    Plan p;
    make_plan(d, p);
    Work wk;
    if (!make_work(p, batch, h, w, wk)) return 0;
    return wk.bytes;
}

extern "C" int straps_regressor_prepare(const straps_regressor_desc_t* d, const float* params, void* prepared, void* stream) {
    const char* bad = check_desc(d);
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
    auto bn_fold = [&](long long bn_off, int c, size_t ss_off) {
        const float* g = params + bn_off;
        return straps_bn_fold(g, g + c, g + 2 * c, g + 3 * c, kBnEps, f(ss_off), f(ss_off) + c, c, stream);
    };
    // stem: fragment-order weights and its folded BatchNorm
    RG_CALL(straps_pack_stem_weight(params + p.stem_w_off, f(p.stem_w), p.cin, stream));
    RG_CALL(bn_fold(p.stem_bn_off, 64, p.stem_ss));
    for (int i = 0; i < p.nconvs; ++i) RG_CALL(bn_fold(p.convs[i]->bn_off, p.convs[i]->cout, p.convs[i]->ss_off));
    if (p.precision == 0) {
        // every layer's bf16x3 forward planes in one launch (ResNet.prepack without the data-gradient layout)
        straps_pack_desc_t table[kMaxConvs];
        for (int i = 0; i < p.nconvs; ++i) {
            const Conv& cv = *p.convs[i];
            table[i].src = params + cv.w_off;
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
            const Conv& cv = *p.convs[i];
            RG_CALL(straps_pack_conv_weight_bf16(params + cv.w_off, (unsigned short*)(pb + p.planes) + cv.first, cv.cout, cv.cin, cv.k, cv.k, stream));
        }
    } else {
        for (int i = 0; i < p.nconvs; ++i) {
            const Conv& cv = *p.convs[i];
            RG_CALL(straps_pack_conv_weight(params + cv.w_off, f(cv.wk_off), cv.cout, cv.cin, cv.k, cv.k, stream));
        }
    }
    // IEF: the repacked fc1 / fc3 views, and copies of everything else the iterations read (the forward never touches `params`)
    RG_CALL(straps_ief_pack(params + p.fc1w_off, params + p.fc3w_off, f(p.w1f), f(p.w1e), f(p.w3), p.F, kNumParams, p.H1, p.H2, kEstLd, stream));
    const struct { size_t dst; long long src, n; } copies[] = {
        {p.fc1b, p.fc1b_off, p.H1}, {p.fc2w, p.fc2w_off, (long long)p.H2 * p.H1}, {p.fc2b, p.fc2b_off, p.H2},
        {p.fc3b, p.fc3b_off, kNumParams}, {p.init, p.init_off, kNumParams}};
    for (const auto& c : copies)
        RG_HIP(hipMemcpyAsync(f(c.dst), params + c.src, c.n * sizeof(float), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(IEF parameters)");
    RG_HIP(hipStreamSynchronize(st), "hipStreamSynchronize");
    return STRAPS_OK;
}

extern "C" int straps_regressor_fwd_infer(const straps_regressor_desc_t* d, const void* prepared, const float* x, int batch, int h, int w,
                                          float* est, int ld_est, float* rotmats, void* workspace, size_t workspace_bytes, void* stream) {
    const char* bad = check_desc(d);
    STRAPS_REQUIRE(!bad, "straps_regressor_fwd_infer: %s", bad);
    STRAPS_REQUIRE(prepared, "straps_regressor_fwd_infer: null pointer `prepared`");
    STRAPS_REQUIRE(x, "straps_regressor_fwd_infer: null pointer `x`");
    STRAPS_REQUIRE(est, "straps_regressor_fwd_infer: null pointer `est`");
    STRAPS_REQUIRE(workspace, "straps_regressor_fwd_infer: null pointer `workspace`");
    STRAPS_REQUIRE(batch > 0, "straps_regressor_fwd_infer: `batch` must be positive (got %d)", batch);
    STRAPS_REQUIRE(h >= 7 && w >= 7, "straps_regressor_fwd_infer: `h` and `w` must be at least 7 (got %d x %d)", h, w);
    STRAPS_REQUIRE(ld_est >= kNumParams, "straps_regressor_fwd_infer: `ld_est` must be >= %d (got %d)", kNumParams, ld_est);
    STRAPS_REQUIRE(((uintptr_t)prepared & (kAlign - 1)) == 0 && ((uintptr_t)workspace & (kAlign - 1)) == 0,
                   "straps_regressor_fwd_infer: `prepared` and `workspace` must be %zu-byte aligned", kAlign);
    STRAPS_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)est & 3) == 0 && ((uintptr_t)rotmats & 3) == 0,
                   "straps_regressor_fwd_infer: `x`, `est` and `rotmats` must be float-aligned");
    Plan p;
    make_plan(d, p);
    Work wk;
    STRAPS_REQUIRE(make_work(p, batch, h, w, wk), "straps_regressor_fwd_infer: input %d x %d is too small for resnet%d", h, w, p.layers);
    STRAPS_REQUIRE(workspace_bytes >= wk.bytes, "straps_regressor_fwd_infer: `workspace_bytes` is %zu, this batch needs %zu (straps_regressor_workspace_bytes)",
                   workspace_bytes, wk.bytes);
    const bool x3 = p.precision == 0, b16 = p.precision == 3;
    const char* pb = (const char*)prepared;
    char* ws = (char*)workspace;
    auto pf = [&](size_t off) { return (const float*)(pb + off); };
    auto wf = [&](size_t off) { return (float*)(ws + off); };
    auto wp = [&](size_t off) { return (unsigned short*)(ws + off); };
    const unsigned short* wplanes = (const unsigned short*)(pb + p.planes);
    const int B = batch, C = p.cin;

    // ---- stem: non-zero map, conv 7x7/s2 with folded BatchNorm + ReLU (encoder_forward, eval), max pool into io[0] ----
    uint32_t* nz = (uint32_t*)(ws + wk.nzmask);
    RG_CALL(straps_stem_nzmask(x, nz, B, C, h, w, stream));
    RG_CALL(straps_stem_fwd(x, pf(p.stem_w), pf(p.stem_ss), pf(p.stem_ss) + 64, 1, wf(wk.stem_out), nullptr, nz, B, C, h, w, stream));
    RG_CALL(straps_maxpool_fwd(wf(wk.stem_out), wf(wk.io[0]), B, wk.Hs, wk.Ws, 64, stream));
    int H = wk.Hp, W = wk.Wp, cur = 0;
    if (x3)      // the pooled input is the only activation split into planes by a pass of its own
        RG_CALL(straps_split3_bf16_cm(wf(wk.io[0]), wp(wk.io_planes[0]), (long long)B * H * W, 64, wk.io_ps, stream));
    if (b16)
        RG_CALL(straps_split_bf16_cm(wf(wk.io[0]), wp(wk.io_planes[0]), (long long)B * H * W, 64, stream));

    // ---- residual stages (encoder_exec._residual_stages, eval without a tape) ----
    for (int ui = 0; ui < p.nunits; ++ui) {
        const Unit& u = p.units[ui];
        const float* in = wf(wk.io[cur]);
        const unsigned short* in3 = (x3 || b16) ? wp(wk.io_planes[cur]) : nullptr;
        const float* idt = in;
        if (u.has_ds) {     // projection: no ReLU, fp32 output only
            const Conv& cv = u.ds;
            const float* ss = pf(cv.ss_off);
            if (x3)
                RG_CALL(straps_conv_fwd_x3(in3, wk.io_ps, wplanes + cv.first, p.ps, ss, ss + cv.cout, nullptr, 0, wf(wk.idt), nullptr,
                                           B, H, W, cv.cin, cv.cout, 1, 1, cv.stride, 0, 0, stream));
            else if (b16)
                RG_CALL(straps_conv_fwd_bf16(in3, wplanes + cv.first, ss, ss + cv.cout, nullptr, 0, wf(wk.idt), nullptr, B, H, W, cv.cin, cv.cout, 1, 1,
                                             cv.stride, 0, 0, stream));
            else
                RG_CALL(straps_conv_fwd(in, pf(cv.wk_off), ss, ss + cv.cout, nullptr, 0, wf(wk.idt), nullptr, B, H, W, cv.cin, cv.cout, 1, 1,
                                        cv.stride, 0, 0, stream));
            idt = wf(wk.idt);
        }
        const float* t = in;
        const unsigned short* t3 = in3;
        long long t_ps = wk.io_ps;
        int th = H, tw = W;
        for (int ci = 0; ci < u.nconv; ++ci) {
            const Conv& cv = u.c[ci];
            const bool last = ci == u.nconv - 1;
            const float* ss = pf(cv.ss_off);
            const float* res = last ? idt : nullptr;
            float* y = last ? wf(wk.io[cur ^ 1]) : ((x3 || b16) ? nullptr : wf(wk.mid[ci]));
            unsigned short* y3 = (x3 || b16) ? (last ? wp(wk.io_planes[cur ^ 1]) : wp(wk.mid[ci])) : nullptr;
            const long long y_ps = last ? wk.io_ps : wk.mid_ps[ci];
            if (x3)      // ReLU outputs write their planes in the epilogue; the fp32 tensor only for a unit's output
                RG_CALL(straps_conv_fwd_x3p(t3, t_ps, wplanes + cv.first, p.ps, ss, ss + cv.cout, res, 1, y, y3, y_ps,
                                            B, th, tw, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0, stream));
            else if (b16)      // the same with one plane
                RG_CALL(straps_conv_fwd_bf16(t3, wplanes + cv.first, ss, ss + cv.cout, res, 1, y, y3, B, th, tw, cv.cin, cv.cout, cv.k, cv.k, cv.stride,
                                             cv.pad, 0, stream));
            else
                RG_CALL(straps_conv_fwd(t, pf(cv.wk_off), ss, ss + cv.cout, res, 1, y, nullptr, B, th, tw, cv.cin, cv.cout, cv.k, cv.k,
                                        cv.stride, cv.pad, 0, stream));
            th = conv_out(th, cv.k, cv.stride, cv.pad);
            tw = conv_out(tw, cv.k, cv.stride, cv.pad);
            t = y;
            t3 = y3;
            t_ps = y_ps;
        }
        H = th;
        W = tw;
        cur ^= 1;
    }

    // ---- global average pool, then the IEF iterations (IEFModule.forward_estimate) ----
    float* feat = wf(wk.feat);
    float* c1 = wf(wk.c1);
    float* ests = wf(wk.ests);
    float* h1 = wf(wk.h1);
    float* h2 = wf(wk.h2);
    const int F = p.F, H1 = p.H1, H2 = p.H2, T = p.iters;
    RG_CALL(straps_gap_fwd(wf(wk.io[cur]), feat, B, H * W, F, stream));
    RG_CALL(straps_broadcast_rows(pf(p.init), kNumParams, ests, kEstLd, (T + 1) * B, stream));
    RG_CALL(straps_linear_fwd(feat, F, pf(p.w1f), F, pf(p.fc1b), nullptr, c1, H1, B, H1, F, 0, stream));
    // with ld_est == 160 the last iteration writes `est` itself (the fc3 epilogue reads its addend with the output's row stride);
    // otherwise it writes the last workspace slot, copied out below
    const bool direct = ld_est == kEstLd;
    for (int it = 0; it < T; ++it) {
        float* est_in = ests + (size_t)it * B * kEstLd;
        float* est_out = direct && it == T - 1 ? est : est_in + (size_t)B * kEstLd;
        RG_CALL(straps_linear_fwd(est_in, kEstLd, pf(p.w1e), kEstLd, nullptr, c1, h1, H1, B, H1, kEstLd, 1, stream));
        RG_CALL(straps_linear_fwd(h1, H1, pf(p.fc2w), H1, pf(p.fc2b), nullptr, h2, H2, B, H2, H1, 1, stream));
        RG_CALL(straps_linear_fwd(h2, H2, pf(p.w3), H2, pf(p.fc3b), est_in, est_out, kEstLd, B, kNumParams, H2, 0, stream));
    }
    if (!direct) RG_CALL(straps_masked_copy(ests + (size_t)T * B * kEstLd, kEstLd, nullptr, 0, est, ld_est, B, kNumParams, 0, stream));
    if (rotmats) RG_CALL(straps_rot6d_fwd(est + 3, ld_est, 24, rotmats, B, stream));
    return STRAPS_OK;
}
