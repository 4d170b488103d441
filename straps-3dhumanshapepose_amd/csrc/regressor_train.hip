// regressor_train.hip -- the train-mode regressor forward and backward behind C entry points (straps_regressor_fwd_train / _bwd,
// include/straps_hip.h), for hosts without torch.
//
// Host scheduling only, like regressor.hip: every launch is an existing entry point of this library, called with the arguments the
// autograd path of SingleInputRegressor in train mode passes from Python (encoder_exec.encoder_forward with a tape,
// IEFModule.forward_estimate, autograd_ops.ief_backward / encoder_backward) with the module's defaults, so estimates, gradients and
// running statistics are bit-identical to the module's.  The one launch of its own (write_table_kernel) only moves the weight-pack
// descriptor table into the workspace: the table lives in the kernel arguments, so nothing is copied from host memory and a
// fwd_train + bwd pair can be captured into a hipGraph.
//
// A Plan adds to the network walk and geometry of regressor_net.h, for one (batch, h, w): every layer's route (fp32-operand 1x1,
// bf16x3 planes, fp32), which forms of each activation the module materialises, and the workspace offsets of the tape and of the
// backward's reused slots.
#include <algorithm>
#include <cstring>

#include "regressor_net.h"

namespace {

constexpr long long kX3fMinRows = 16384;    // encoder_exec.X3F_MIN_ROWS
constexpr size_t kNone = ~(size_t)0;        // "this form of a tensor is not materialised"

// one convolution with its training route, tensor forms and tape
struct Layer : Conv, Extent {
    long long rows;                   // batch * Ho * Wo
    bool fmode;                       // fp32-operand route (encoder_exec.x3f_mode)
    bool keep, planes, defer, bits;   // output forms: fp32, planes, BatchNorm deferred into the consumer, ReLU bits
    bool keep_grad;                   // autograd_ops keep(): does anything read the fp32 gradient of the raw output
    int nblk;                         // forward statistics blocks
    // input activation (workspace offsets; kNone = not materialised) and the deferred BatchNorm applied in the operand path
    size_t x, x3;
    long long x_ps;
    const Layer* a_bn;
    // tape
    size_t raw, ss, out, out3, bitsb;
    long long out_ps;
};

struct Plan : Net {
    bool x3;
    int B, stem_nblk;
    Geometry geo;
    Layer lay[kMaxConvs];             // Net::convs with their training state
    bool pool_planes;
    long long amax;                   // largest activation / raw output (elements)
    // workspace (bytes): packed weights, tape, forward scratch, backward slots
    size_t wstem, wsd, table, one, krsc, crsk, w1f, w1e, w3;
    size_t nz, stem_raw, stem_ss, pool, pool3, idx;
    long long pool_ps;
    size_t feat, c1, ests, h1s, h2s, fpart;
    size_t g[2], dz, dskip, dt, draw, draw3, drawd, drawd3, part, bnws, wgws, tact, sdraw, swgws, dgb, dests, dh2s, dh1s, dc1, dfeat;
    size_t bytes;
    const Layer& unit_out(int ui) const { return lay[units[ui].c[units[ui].nconv - 1]]; }      // a unit's last convolution
};

bool x3f_mode(const Plan& p, const Layer& cv) {
    if (!p.x3 || !straps_conv_x3f_supported(cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad)) return false;
    return (long long)p.B * cv.Ho * cv.Wo >= kX3fMinRows;
}

// (fp32, planes) forms an activation must exist in for the convolution that reads it (encoder_exec._residual_stages.needs)
void needs(const Plan& p, const Layer& cv, bool& f32, bool& planes) {
    if (x3f_mode(p, cv)) { f32 = true; planes = false; return; }
    f32 = !straps_conv_wgrad_x3_on_planes(p.B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad);
    planes = true;
}

// routes, tensor forms and workspace offsets for one (batch, h, w) on top of make_net; false if the input is too small for the network
bool make_plan(Plan& p, int B, int H, int W) {
    if (!make_geometry(p, B, H, W, p.geo)) return false;
    p.x3 = p.precision == 0;
    p.B = B;
    for (int i = 0; i < p.nconvs; ++i) {
        static_cast<Conv&>(p.lay[i]) = p.convs[i];
        static_cast<Extent&>(p.lay[i]) = p.geo.e[i];
    }
    size_t b = 0;
    auto take = [&](size_t bytes) { const size_t o = b; b = align_up(b + (bytes ? bytes : 1)); return o; };
    auto f32s = [&](long long n) { return take((size_t)n * sizeof(float)); };
    auto planes = [&](long long n) { return take(3 * (size_t)round8(n) * sizeof(unsigned short)); };
    // ---- packed weights (written by fwd_train; the stem's data-gradient packing by bwd) ----
    p.wstem = f32s((long long)straps_stem_weight_floats(p.cin));
    p.wsd = p.cin <= STRAPS_STEM_DGRAD_MAX_CIN ? f32s((long long)straps_stem_dgrad_weight_floats(p.cin)) : kNone;
    p.table = take(kMaxConvs * sizeof(straps_pack_desc_t));
    p.one = f32s(1);
    if (p.x3) { p.krsc = take(3 * (size_t)p.ps * sizeof(unsigned short)); p.crsk = take(3 * (size_t)p.ps * sizeof(unsigned short)); }
    else { p.krsc = f32s(p.conv_total); p.crsk = f32s(p.conv_total); }
    p.w1f = f32s((long long)p.H1 * p.F);
    p.w1e = f32s((long long)p.H1 * kEstLd);
    p.w3 = f32s((long long)(kNumParams + 31) / 32 * 32 * p.H2);
    // ---- stem tape ----
    const long long stem_n = (long long)B * p.geo.Hs * p.geo.Ws * 64, pool_n = (long long)B * p.geo.Hp * p.geo.Wp * 64;
    p.nz = take(straps_stem_nzmask_words(B, p.cin, H, W) * sizeof(uint32_t));
    p.stem_raw = f32s(stem_n);
    p.stem_ss = f32s(4 * 64);
    p.pool = f32s(pool_n);
    p.idx = take((size_t)pool_n);
    p.stem_nblk = straps_stem_stat_blocks(B, H, W);
    long long fpart = (long long)p.stem_nblk * 64 * 2;
    p.amax = pool_n;
    {   // the pooled output's planes unless every reader takes the fp32 tensor (encoder_forward)
        const Unit& u0 = p.units[0];
        bool all = x3f_mode(p, p.lay[u0.c[0]]) && (!u0.has_ds || x3f_mode(p, p.lay[u0.ds]));
        p.pool_planes = p.x3 && !all;
        p.pool3 = p.pool_planes ? planes(pool_n) : kNone;
        p.pool_ps = p.pool_planes ? round8(pool_n) : 0;
    }
    // ---- residual stages: every convolution's tape (encoder_exec._residual_stages / conv_bn / _bn_train_finish) ----
    long long part_d = 1, bnws = straps_bn_bwd_workspace_bytes(stem_n, 64), wgws = 4;
    size_t in = p.pool, in3 = p.pool3;
    long long in_ps = p.pool_ps;
    auto tape = [&](Layer& cv) -> bool {
        const int ch = cv.H, cw = cv.W;
        cv.rows = (long long)B * cv.Ho * cv.Wo;
        cv.fmode = x3f_mode(p, cv);
        cv.nblk = cv.fmode ? straps_conv_x3f_stat_blocks(B, ch, cw, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0)
                 : p.x3    ? straps_conv_x3_stat_blocks(B, ch, cw, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0)
                           : straps_conv_stat_blocks(B, cv.Ho, cv.Wo, cv.cout, cv.k * cv.k * cv.cin, 0);
        if (cv.nblk <= 0) return false;
        fpart = std::max(fpart, (long long)cv.nblk * cv.cout * 2);
        const long long n = cv.rows * cv.cout;
        p.amax = std::max(p.amax, n);
        bnws = std::max(bnws, (long long)straps_bn_bwd_workspace_bytes(cv.rows, cv.cout));
        wgws = std::max(wgws, (long long)(cv.fmode ? straps_conv_wgrad_x3f_workspace_bytes(B, ch, cw, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad)
                                                   : straps_conv_wgrad_workspace_bytes(B, ch, cw, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad)));
        if (p.x3) {     // the data gradient's BatchNorm partials of the layer in front (double [blocks][cin][2])
            const int nb = cv.fmode ? straps_conv_dgrad_x3f_bn_blocks(B, ch, cw, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0)
                                    : straps_conv_dgrad_x3_bn_blocks(B, ch, cw, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0);
            part_d = std::max(part_d, (long long)nb * cv.cin * 2);
        }
        cv.raw = f32s(n);
        cv.ss = f32s(4LL * cv.cout);
        return true;
    };
    for (int ui = 0; ui < p.nunits; ++ui) {
        const Unit& u = p.units[ui];
        if (u.has_ds) {     // projection: BatchNorm without ReLU, fp32 output (the identity)
            Layer& cv = p.lay[u.ds];
            if (!tape(cv)) return false;
            cv.x = in; cv.x3 = in3; cv.x_ps = in_ps; cv.a_bn = nullptr;
            cv.keep = true; cv.planes = false; cv.defer = false; cv.bits = false;
            cv.out = f32s(cv.rows * cv.cout); cv.out3 = kNone; cv.out_ps = 0; cv.bitsb = kNone;
        }
        size_t t = in, t3 = in3;
        long long t_ps = in_ps;
        const Layer* a_bn = nullptr;
        for (int ci = 0; ci < u.nconv; ++ci) {
            Layer& cv = p.lay[u.c[ci]];
            if (!tape(cv)) return false;
            cv.x = t; cv.x3 = t3; cv.x_ps = t_ps; cv.a_bn = a_bn;
            bool keep = true, pl = true, defer = false;
            if (p.x3 && !cv.last) {
                needs(p, p.lay[u.c[ci + 1]], keep, pl);
                defer = keep && !pl;
            } else if (p.x3) {
                pl = false;
                if (ui + 1 < p.nunits) {
                    const Unit& nx = p.units[ui + 1];
                    bool f, q;
                    needs(p, p.lay[nx.c[0]], f, q);
                    pl = q;
                    if (nx.has_ds) { needs(p, p.lay[nx.ds], f, q); pl = pl || q; }
                }
            }
            cv.defer = defer;
            cv.bits = p.x3 && cv.last;
            if (defer) {            // the raw output is the consumer's input; its BatchNorm + ReLU run in that layer's operand path
                cv.keep = false; cv.planes = false;
                cv.out = kNone; cv.out3 = kNone; cv.out_ps = 0; cv.bitsb = kNone;
                t = cv.raw; t3 = kNone; t_ps = 0; a_bn = &cv;
            } else {
                if (!p.x3) { keep = true; pl = false; }
                else keep = keep || !pl;
                cv.keep = keep; cv.planes = pl;
                cv.out = keep ? f32s(cv.rows * cv.cout) : kNone;
                cv.out3 = pl ? planes(cv.rows * cv.cout) : kNone;
                cv.out_ps = pl ? round8(cv.rows * cv.cout) : 0;
                cv.bitsb = cv.bits ? take((size_t)cv.rows * (cv.cout / 32) * sizeof(uint32_t)) : kNone;
                t = cv.out; t3 = cv.out3; t_ps = cv.out_ps; a_bn = nullptr;
            }
        }
        in = t; in3 = t3; in_ps = t_ps;
    }
    // autograd_ops.encoder_backward keep(): the fp32 gradient of a raw output is needed unless its weight gradient runs on planes
    for (int i = 0; i < p.nconvs; ++i) {
        Layer& cv = p.lay[i];
        cv.keep_grad = !p.x3 || cv.fmode || !straps_conv_wgrad_x3_on_planes(B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad);
    }
    p.feat = f32s((long long)B * p.F);
    p.c1 = f32s((long long)B * p.H1);
    p.ests = f32s((long long)(p.iters + 1) * B * kEstLd);
    p.h1s = f32s((long long)p.iters * B * p.H1);
    p.h2s = f32s((long long)p.iters * B * p.H2);
    p.fpart = f32s(fpart);
    // ---- backward slots, reused by every unit ----
    for (int i = 0; i < 2; ++i) p.g[i] = f32s(p.amax);
    p.dz = f32s(p.amax);
    p.dskip = f32s(p.amax);
    p.dt = f32s(p.amax);
    p.draw = f32s(p.amax);
    p.drawd = f32s(p.amax);
    p.draw3 = p.x3 ? planes(p.amax) : kNone;
    p.drawd3 = p.x3 ? planes(p.amax) : kNone;
    p.part = take((size_t)part_d * sizeof(double));
    p.bnws = take((size_t)bnws);
    p.wgws = take((size_t)wgws);
    p.tact = take(straps_stem_tiles(B, H, W));
    p.sdraw = f32s(stem_n);
    p.swgws = take(straps_stem_wgrad_workspace_bytes(B, p.cin, H, W));
    p.dgb = f32s(2 * 2048);
    p.dests = f32s((long long)(p.iters + 1) * B * kEstLd);
    p.dh2s = f32s((long long)p.iters * B * p.H2);
    p.dh1s = f32s((long long)p.iters * B * p.H1);
    p.dc1 = f32s((long long)B * p.H1);
    p.dfeat = f32s((long long)B * p.F);
    p.bytes = b;
    return true;
}

struct PackTable {
    straps_pack_desc_t d[kMaxConvs];
};

// the descriptor table of the batched weight pack (and the constant 1.0 the IEF bias gradients contract with) from the kernel
// arguments into the workspace
__global__ __launch_bounds__(64) void write_table_kernel(PackTable t, int n, straps_pack_desc_t* dst, float* one) {
    const int i = threadIdx.x;
    if (i < n) dst[i] = t.d[i];
    if (i == 0) *one = 1.0f;
}

struct Ws {
    char* base;
    float* f(size_t off) const { return off == kNone ? nullptr : (float*)(base + off); }
    unsigned short* h(size_t off) const { return off == kNone ? nullptr : (unsigned short*)(base + off); }
    unsigned* u(size_t off) const { return off == kNone ? nullptr : (unsigned*)(base + off); }
};

// the argument checks fwd_train and bwd share beyond check_args; also walks the plan for this input
int check_common(const char* fn, const straps_regressor_desc_t* d, const float* params, const float* x, int batch, int h, int w,
                 const void* workspace, Plan& p) {
    RG_CALL(check_args(fn, d, true, x, batch, h, w, workspace));
    STRAPS_REQUIRE(params, "%s: null pointer `params`", fn);
    STRAPS_REQUIRE(((uintptr_t)params & 15) == 0, "%s: `params` must be 16-byte aligned", fn);
    make_net(d, p);
    STRAPS_REQUIRE(make_plan(p, batch, h, w), "%s: input %d x %d is too small for resnet%d", fn, h, w, p.layers);
    return STRAPS_OK;
}

int finalize(const float* params, float* bn_state, const float* part, int nblk, int c, long long rows, long long gb, long long rs, float* ss,
             hipStream_t st) {
    return straps_bn_stats_finalize(part, nblk, c, rows, params + gb, params + gb + c, kBnEps, kBnMomentum, bn_state + rs, bn_state + rs + c,
                                    ss, ss + c, ss + 2 * c, ss + 3 * c, st);
}

}  // namespace

extern "C" size_t straps_regressor_train_param_floats(const straps_regressor_desc_t* d) {
    if (check_desc(d, true)) return 0;
    Net n;
    make_net(d, n);
    return (size_t)n.train_floats;
}

extern "C" size_t straps_regressor_bn_state_floats(const straps_regressor_desc_t* d) {
    if (check_desc(d, true)) return 0;
    Net n;
    make_net(d, n);
    return (size_t)n.bn_floats;
}

extern "C" size_t straps_regressor_train_workspace_bytes(const straps_regressor_desc_t* d, int batch, int h, int w) {
    if (check_desc(d, true)) return 0;
    Plan p;
    make_net(d, p);
    if (!make_plan(p, batch, h, w)) return 0;
    return p.bytes;
}

extern "C" int straps_regressor_fwd_train(const straps_regressor_desc_t* d, const float* params, float* bn_state, const float* init_est,
                                          const float* x, int batch, int h, int w, float* est, int ld_est, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    static const char* fn = "straps_regressor_fwd_train";
    Plan p;
    RG_CALL(check_common(fn, d, params, x, batch, h, w, workspace, p));
    STRAPS_REQUIRE(bn_state, "%s: null pointer `bn_state`", fn);
    STRAPS_REQUIRE(init_est, "%s: null pointer `init_est`", fn);
    STRAPS_REQUIRE(est, "%s: null pointer `est`", fn);
    STRAPS_REQUIRE(ld_est >= kNumParams, "%s: `ld_est` must be >= %d (got %d)", fn, kNumParams, ld_est);
    STRAPS_REQUIRE(((uintptr_t)bn_state & 3) == 0 && ((uintptr_t)init_est & 3) == 0 && ((uintptr_t)est & 3) == 0,
                   "%s: `bn_state`, `init_est` and `est` must be float-aligned", fn);
    STRAPS_REQUIRE(workspace_bytes >= p.bytes, "%s: `workspace_bytes` is %zu, this batch needs %zu (straps_regressor_train_workspace_bytes)", fn,
                   workspace_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    const Ws ws{(char*)workspace};
    const int B = batch, C = p.cin, F = p.F, H1 = p.H1, H2 = p.H2;
    const bool x3 = p.x3;
    unsigned short* krsc3 = ws.h(p.krsc);
    float* krsc = ws.f(p.krsc);

    // ---- weights: the stem's fragment order, every convolution in one batched pack (ResNet.prepack, both layouts), the IEF packing ----
    RG_CALL(straps_pack_stem_weight(params + p.stem.w_off, ws.f(p.wstem), C, stream));
    PackTable tbl;
    memset(&tbl, 0, sizeof(tbl));
    for (int i = 0; i < p.nconvs; ++i) {
        const Conv& cv = p.convs[i];
        straps_pack_desc_t& e = tbl.d[i];
        e.src = params + cv.w_off;
        e.dst_krsc = x3 ? nullptr : ws.f(p.krsc) + cv.first;
        e.dst_crsk = x3 ? nullptr : ws.f(p.crsk) + cv.first;
        e.o = cv.cout; e.c = cv.cin; e.r = cv.k; e.s = cv.k;
        e.first = cv.first;
    }
    straps_pack_desc_t* table = (straps_pack_desc_t*)(ws.base + p.table);
    hipLaunchKernelGGL(write_table_kernel, dim3(1), dim3(64), 0, st, tbl, p.nconvs, table, ws.f(p.one));
    STRAPS_CHECK_LAUNCH("write_table_kernel");
    if (x3) RG_CALL(straps_pack_conv_weights_batched_x3(table, p.nconvs, p.conv_total, krsc3, ws.h(p.crsk), p.ps, stream));
    else RG_CALL(straps_pack_conv_weights_batched(table, p.nconvs, p.conv_total, stream));
    RG_CALL(straps_ief_pack(params + p.ief.fc1w, params + p.ief.fc3w, ws.f(p.w1f), ws.f(p.w1e), ws.f(p.w3), F, kNumParams, H1, H2, kEstLd, stream));

    // ---- stem: raw conv + statistics, BatchNorm + ReLU + max pool in one pass (encoder_forward with a tape) ----
    uint32_t* nz = (uint32_t*)(ws.base + p.nz);
    float* part = ws.f(p.fpart);
    float* sss = ws.f(p.stem_ss);
    RG_CALL(straps_stem_nzmask(x, nz, B, C, h, w, stream));
    RG_CALL(straps_stem_fwd(x, ws.f(p.wstem), nullptr, nullptr, 0, ws.f(p.stem_raw), part, nz, B, C, h, w, stream));
    RG_CALL(finalize(params, bn_state, part, p.stem_nblk, 64, (long long)B * p.geo.Hs * p.geo.Ws, p.stem.gb_off, p.stem.rs_off, sss, st));
    if (p.pool_planes)
        RG_CALL(straps_bn_relu_maxpool_fwd_x3(ws.f(p.stem_raw), sss, sss + 64, ws.f(p.pool), (uint8_t*)(ws.base + p.idx), ws.h(p.pool3), p.pool_ps,
                                              B, p.geo.Hs, p.geo.Ws, 64, stream));
    else
        RG_CALL(straps_bn_relu_maxpool_fwd(ws.f(p.stem_raw), sss, sss + 64, ws.f(p.pool), (uint8_t*)(ws.base + p.idx), B, p.geo.Hs, p.geo.Ws, 64, stream));

    // ---- residual stages (conv_bn in training mode with a tape) ----
    auto conv_fwd = [&](const Layer& cv) -> int {
        const float* sa = cv.a_bn ? ws.f(cv.a_bn->ss) : nullptr;
        if (cv.fmode)
            return straps_conv_fwd_x3f(ws.f(cv.x), sa, sa ? sa + cv.a_bn->cout : nullptr, cv.a_bn ? 1 : 0, krsc3 + cv.first, p.ps, nullptr, nullptr,
                                       nullptr, 0, ws.f(cv.raw), part, B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0, stream);
        if (x3)
            return straps_conv_fwd_x3(ws.h(cv.x3), cv.x_ps, krsc3 + cv.first, p.ps, nullptr, nullptr, nullptr, 0, ws.f(cv.raw), part,
                                      B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0, stream);
        return straps_conv_fwd(ws.f(cv.x), krsc + cv.first, nullptr, nullptr, nullptr, 0, ws.f(cv.raw), part, B, cv.H, cv.W, cv.cin, cv.cout,
                               cv.k, cv.k, cv.stride, cv.pad, 0, stream);
    };
    auto conv_bn = [&](const Layer& cv, const float* residual) -> int {
        RG_CALL(conv_fwd(cv));
        float* ss = ws.f(cv.ss);
        RG_CALL(finalize(params, bn_state, part, cv.nblk, cv.cout, cv.rows, cv.gb_off, cv.rs_off, ss, st));
        if (cv.defer) return STRAPS_OK;
        if (x3 && cv.relu) {
            if (cv.bits)
                return straps_bn_apply_bits_x3(ws.f(cv.raw), ss, ss + cv.cout, residual, ws.f(cv.out), ws.h(cv.out3), cv.out_ps, ws.u(cv.bitsb),
                                               cv.rows, cv.cout, stream);
            return straps_bn_apply_x3(ws.f(cv.raw), ss, ss + cv.cout, residual, 1, ws.f(cv.out), ws.h(cv.out3), cv.out_ps, cv.rows, cv.cout, stream);
        }
        return straps_bn_apply(ws.f(cv.raw), ss, ss + cv.cout, residual, cv.relu ? 1 : 0, ws.f(cv.out), cv.rows, cv.cout, stream);
    };
    for (int ui = 0; ui < p.nunits; ++ui) {
        const Unit& u = p.units[ui];
        const float* idt = ws.f(p.lay[u.c[0]].x);
        if (u.has_ds) {
            RG_CALL(conv_bn(p.lay[u.ds], nullptr));
            idt = ws.f(p.lay[u.ds].out);
        }
        for (int ci = 0; ci < u.nconv; ++ci) RG_CALL(conv_bn(p.lay[u.c[ci]], p.lay[u.c[ci]].last ? idt : nullptr));
    }

    // ---- global average pool, then the IEF iterations with every iteration's activations kept (the backward never reads the last
    // estimate slot: the last iteration may write `est` itself) ----
    RG_CALL(ief_forward(p, B, ws.f(p.unit_out(p.nunits - 1).out), p.geo.Hf * p.geo.Wf, init_est, ws.f(p.w1f), ws.f(p.w1e), params + p.ief.fc1b,
                        params + p.ief.fc2w, params + p.ief.fc2b, ws.f(p.w3), params + p.ief.fc3b, ws.f(p.feat), ws.f(p.c1), ws.f(p.ests),
                        ws.f(p.h1s), (long long)B * H1, ws.f(p.h2s), (long long)B * H2, est, ld_est, stream));
    return STRAPS_OK;
}

extern "C" int straps_regressor_bwd(const straps_regressor_desc_t* d, const float* params, const float* x, int batch, int h, int w,
                                    const float* dest, int ld_dest, float* grads, float* dx, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    static const char* fn = "straps_regressor_bwd";
    Plan p;
    RG_CALL(check_common(fn, d, params, x, batch, h, w, workspace, p));
    STRAPS_REQUIRE(dest, "%s: null pointer `dest`", fn);
    STRAPS_REQUIRE(ld_dest >= kNumParams, "%s: `ld_dest` must be >= %d (got %d)", fn, kNumParams, ld_dest);
    STRAPS_REQUIRE(((uintptr_t)dest & 3) == 0 && ((uintptr_t)grads & 3) == 0 && ((uintptr_t)dx & 3) == 0,
                   "%s: `dest`, `grads` and `dx` must be float-aligned", fn);
    STRAPS_REQUIRE(!dx || p.cin <= STRAPS_STEM_DGRAD_MAX_CIN, "%s: `dx` needs `in_channels` <= %d (got %d)", fn, STRAPS_STEM_DGRAD_MAX_CIN, p.cin);
    STRAPS_REQUIRE(workspace_bytes >= p.bytes, "%s: `workspace_bytes` is %zu, this batch needs %zu (straps_regressor_train_workspace_bytes)", fn,
                   workspace_bytes, p.bytes);
    const Ws ws{(char*)workspace};
    const int B = batch, C = p.cin, F = p.F, H1 = p.H1, H2 = p.H2, T = p.iters, P = kNumParams;
    const bool x3 = p.x3, pg = grads != nullptr;
    const unsigned short* crsk3 = ws.h(p.crsk);
    const float* crsk = ws.f(p.crsk);
    float* dgb = ws.f(p.dgb);          // dgamma / dbeta nobody reads (no parameter gradients asked for)
    auto dgamma = [&](long long gb) { return pg ? grads + gb : dgb; };
    auto dbeta = [&](long long gb, int c) { return pg ? grads + gb + c : dgb + 2048; };

    // ---- IEF (autograd_ops.ief_backward): the incoming gradient into its slot, three GEMMs per iteration, one launch for the rest ----
    float* dests = ws.f(p.dests);
    float* dh2s = ws.f(p.dh2s);
    float* dh1s = ws.f(p.dh1s);
    float* dc1 = ws.f(p.dc1);
    float* dfeat = ws.f(p.dfeat);
    const float* ests = ws.f(p.ests);
    const float* h1s = ws.f(p.h1s);
    const float* h2s = ws.f(p.h2s);
    RG_CALL(straps_masked_copy(dest, ld_dest, nullptr, 0, dests + (size_t)T * B * kEstLd, kEstLd, B, P, 0, stream));
    auto gd = [](const float* a, long long sam, long long sak, const float* b, long long sbk, long long sbn, float* c, int ldc, int m, int n, int k) {
        straps_gemm_desc_t g;
        memset(&g, 0, sizeof(g));
        g.a = a; g.sam = sam; g.sak = sak; g.b = b; g.sbk = sbk; g.sbn = sbn; g.c = c; g.ldc = ldc; g.m = m; g.n = n; g.k = k;
        return g;
    };
    for (int it = T - 1; it >= 0; --it) {
        float* dnext = dests + (size_t)(it + 1) * B * kEstLd;
        float* dh2 = dh2s + (size_t)it * B * H2;
        float* dh1 = dh1s + (size_t)it * B * H1;
        straps_gemm_desc_t g = gd(dnext, kEstLd, 1, params + p.ief.fc3w, H2, 1, dh2, H2, B, H2, P);
        g.mask = h2s + (size_t)it * B * H2; g.ldmask = H2;
        RG_CALL(straps_gemm_multi(&g, 1, stream));
        g = gd(dh2, H2, 1, params + p.ief.fc2w, H1, 1, dh1, H1, B, H1, H2);
        g.mask = h1s + (size_t)it * B * H1; g.ldmask = H1;
        g.c2 = dc1; g.ldc2 = H1; g.accumulate2 = it != T - 1;
        RG_CALL(straps_gemm_multi(&g, 1, stream));
        g = gd(dh1, H1, 1, ws.f(p.w1e), kEstLd, 1, dests + (size_t)it * B * kEstLd, kEstLd, B, P, H1);
        g.addend = dnext; g.ldadd = kEstLd;
        RG_CALL(straps_gemm_multi(&g, 1, stream));
    }
    if (!pg) {
        const straps_gemm_desc_t g = gd(dc1, H1, 1, ws.f(p.w1f), F, 1, dfeat, F, B, F, H1);
        RG_CALL(straps_gemm_multi(&g, 1, stream));
    } else {
        const int KB = T * B;
        const float* one = ws.f(p.one);
        const straps_gemm_desc_t g[8] = {
            gd(dh2s, 1, H2, h1s, H1, 1, grads + p.ief.fc2w, H1, H2, H1, KB),
            gd(dc1, 1, H1, ws.f(p.feat), F, 1, grads + p.ief.fc1w, F + P, H1, F, B),
            gd(dh1s, 1, H1, ests, kEstLd, 1, grads + p.ief.fc1w + F, F + P, H1, P, KB),
            gd(dests + (size_t)B * kEstLd, 1, kEstLd, h2s, H2, 1, grads + p.ief.fc3w, H2, P, H2, KB),
            gd(dc1, H1, 1, ws.f(p.w1f), F, 1, dfeat, F, B, F, H1),
            gd(one, 0, 0, dh2s, H2, 1, grads + p.ief.fc2b, H2, 1, H2, KB),
            gd(one, 0, 0, dests + (size_t)B * kEstLd, kEstLd, 1, grads + p.ief.fc3b, P, 1, P, KB),
            gd(one, 0, 0, dc1, H1, 1, grads + p.ief.fc1b, H1, 1, H1, B)};
        RG_CALL(straps_gemm_multi(g, 8, stream));
    }

    // ---- encoder (autograd_ops.encoder_backward, one stream) ----
    // gradient slots: g[cur] the incoming gradient of a unit's output, g[cur ^ 1] that of its input; draw / drawd the BatchNorm
    // backward outputs (+ planes); dt the inner data gradients; dskip the projection's data gradient; dz the masked copy (fp32 route)
    double* part = (double*)(ws.base + p.part);
    void* bnws = ws.base + p.bnws;
    void* wgws = ws.base + p.wgws;
    const Layer* pending = nullptr;     // the BatchNorm whose backward sums the last data gradient accumulated (rec['bwd_partials'])
    int pending_nblk = 0;
    int cur = 0;
    RG_CALL(straps_gap_bwd(dfeat, ws.f(p.g[cur]), B, p.geo.Hf * p.geo.Wf, F, stream));

    // BatchNorm (+ ReLU) backward of one layer (_bn_bwd); out_off / out3_off: the slots of draw and its planes
    auto bn_bwd = [&](const Layer& cv, const float* dy, bool masked, float* dz, const unsigned* mask_bits, size_t out_off, size_t out3_off) -> int {
        const float* ss = ws.f(cv.ss);
        const int c = cv.cout;
        const bool sink = x3 && !cv.fmode;
        float* draw = (cv.keep_grad || !sink) ? ws.f(out_off) : nullptr;
        unsigned short* planes = sink ? ws.h(out3_off) : nullptr;
        const long long ps = sink ? round8(cv.rows * c) : 0;
        const bool from_raw = masked && !cv.last;
        const unsigned* bits = mask_bits ? mask_bits : (masked && !from_raw ? ws.u(cv.bitsb) : nullptr);
        const bool fused = pending == &cv && masked;
        if (pending == &cv) pending = nullptr;
        float* dg = dgamma(cv.gb_off);
        float* db = dbeta(cv.gb_off, c);
        if (bits) {
            if (fused)
                return straps_bn_bwd_finish_bits_x3(dy, bits, ws.f(cv.raw), ss + 2 * c, ss + 3 * c, params + cv.gb_off, dg, db, draw, planes, ps, part,
                                                    pending_nblk, bnws, cv.rows, c, 0, stream);
            return straps_bn_bwd_bits_x3(dy, bits, ws.f(cv.raw), ss + 2 * c, ss + 3 * c, params + cv.gb_off, dg, db, draw, planes, ps, bnws,
                                         cv.rows, c, 0, stream);
        }
        if (fused)
            return straps_bn_bwd_finish_x3(dy, from_raw ? nullptr : ws.f(cv.out), ws.f(cv.raw), ss + 2 * c, ss + 3 * c, params + cv.gb_off,
                                           from_raw ? ss : nullptr, from_raw ? ss + c : nullptr, dg, db, draw, dz, planes, ps, part, pending_nblk, bnws,
                                           cv.rows, c, 0, stream);
        return straps_bn_bwd_x3(dy, masked && !from_raw ? ws.f(cv.out) : nullptr, ws.f(cv.raw), ss + 2 * c, ss + 3 * c, params + cv.gb_off,
                                from_raw ? ss : nullptr, from_raw ? ss + c : nullptr, dg, db, draw, dz, planes, ps, bnws, cv.rows, c, 0, stream);
    };
    // weight gradient of one layer (_conv_wgrad); draw_off / draw3_off: its output gradient
    auto wgrad = [&](const Layer& cv, size_t draw_off, size_t draw3_off) -> int {
        if (!pg) return STRAPS_OK;
        float* dw = grads + cv.w_off;
        if (cv.fmode) {
            const float* sa = cv.a_bn ? ws.f(cv.a_bn->ss) : nullptr;
            return straps_conv_wgrad_x3f(ws.f(cv.x), sa, sa ? sa + cv.a_bn->cout : nullptr, cv.a_bn ? 1 : 0, ws.f(draw_off), dw, wgws, B, cv.H, cv.W,
                                         cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0, stream);
        }
        if (x3)
            return straps_conv_wgrad_x3(ws.f(cv.x), cv.keep_grad ? ws.f(draw_off) : nullptr, ws.h(cv.x3), cv.x_ps, ws.h(draw3_off), round8(cv.rows * cv.cout),
                                        dw, wgws, B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0, stream);
        return straps_conv_wgrad(ws.f(cv.x), ws.f(draw_off), dw, wgws, B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0, stream);
    };
    // data gradient of one layer (_conv_dgrad); bn_next: the BatchNorm whose output it read (bf16x3: its backward sums ride along)
    auto dgrad = [&](const Layer& cv, size_t draw_off, size_t draw3_off, const float* addend, const unsigned* addend_bits, const Layer* bn_next,
                     float* out) -> int {
        const long long gps = round8(cv.rows * cv.cout);
        if (cv.fmode) {
            const float *raw = nullptr, *msc = nullptr, *msh = nullptr, *mean = nullptr, *invstd = nullptr;
            const unsigned* nbits = nullptr;
            double* prt = nullptr;
            int nblk = 0;
            if (bn_next) {
                const float* ssn = ws.f(bn_next->ss);
                const int cn = bn_next->cout;
                const bool from_raw = !bn_next->last;
                nbits = from_raw ? nullptr : ws.u(bn_next->bitsb);
                if (from_raw || nbits) {
                    nblk = straps_conv_dgrad_x3f_bn_blocks(B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0);
                    prt = part;
                    raw = ws.f(bn_next->raw); mean = ssn + 2 * cn; invstd = ssn + 3 * cn;
                    if (from_raw) { msc = ssn; msh = ssn + cn; }
                }
            }
            RG_CALL(straps_conv_dgrad_x3f(ws.f(draw_off), crsk3 + cv.first, p.ps, addend, addend_bits, out, B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k,
                                          cv.stride, cv.pad, 0, raw, nbits, msc, msh, mean, invstd, prt, stream));
            if (prt) { pending = bn_next; pending_nblk = nblk; }
            return STRAPS_OK;
        }
        if (x3) {
            const unsigned short* g3 = ws.h(draw3_off);
            const unsigned short* w3 = crsk3 + cv.first;
            if (bn_next) {
                const float* ssn = ws.f(bn_next->ss);
                const int cn = bn_next->cout;
                const bool from_raw = !bn_next->last;
                const int nblk = straps_conv_dgrad_x3_bn_blocks(B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0);
                const unsigned* nbits = from_raw ? nullptr : ws.u(bn_next->bitsb);
                if (addend_bits || nbits)
                    RG_CALL(straps_conv_dgrad_x3_bn_bits(g3, gps, w3, p.ps, addend, out, B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0,
                                                         ws.f(bn_next->raw), (from_raw || nbits) ? nullptr : ws.f(bn_next->out),
                                                         from_raw ? ssn : nullptr, from_raw ? ssn + cn : nullptr, ssn + 2 * cn, ssn + 3 * cn, part,
                                                         addend_bits, nbits, stream));
                else
                    RG_CALL(straps_conv_dgrad_x3_bn(g3, gps, w3, p.ps, addend, out, B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0,
                                                    ws.f(bn_next->raw), from_raw ? nullptr : ws.f(bn_next->out), from_raw ? ssn : nullptr,
                                                    from_raw ? ssn + cn : nullptr, ssn + 2 * cn, ssn + 3 * cn, part, stream));
                pending = bn_next;
                pending_nblk = nblk;
                return STRAPS_OK;
            }
            if (addend_bits)
                return straps_conv_dgrad_x3_bits(g3, gps, w3, p.ps, addend, out, B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0,
                                                 addend_bits, stream);
            return straps_conv_dgrad_x3(g3, gps, w3, p.ps, addend, out, B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0, stream);
        }
        return straps_conv_dgrad(ws.f(draw_off), crsk + cv.first, addend, out, B, cv.H, cv.W, cv.cin, cv.cout, cv.k, cv.k, cv.stride, cv.pad, 0, stream);
    };
    for (int ui = p.nunits - 1; ui >= 0; --ui) {
        const Unit& u = p.units[ui];
        const Layer* prev_last = ui > 0 ? &p.unit_out(ui - 1) : nullptr;
        const Layer& lc = p.unit_out(ui);
        const float* dy = ws.f(p.g[cur]);
        const unsigned* ubits = x3 ? ws.u(lc.bitsb) : nullptr;
        const float* dz = dy;
        if (ubits) {
            RG_CALL(bn_bwd(lc, dy, true, nullptr, nullptr, p.draw, p.draw3));
        } else {
            RG_CALL(bn_bwd(lc, dy, true, ws.f(p.dz), nullptr, p.draw, p.draw3));
            dz = ws.f(p.dz);
        }
        RG_CALL(wgrad(lc, p.draw, p.draw3));
        const float* dskip = dz;
        const unsigned* dskip_bits = nullptr;
        if (u.has_ds) {
            const Layer& ds = p.lay[u.ds];
            RG_CALL(bn_bwd(ds, dz, false, nullptr, ubits, p.drawd, p.drawd3));
            RG_CALL(wgrad(ds, p.drawd, p.drawd3));
            RG_CALL(dgrad(ds, p.drawd, p.drawd3, nullptr, nullptr, nullptr, ws.f(p.dskip)));
            dskip = ws.f(p.dskip);
        } else {
            dskip_bits = ubits;
        }
        for (int ci = u.nconv - 1; ci > 0; --ci) {
            const Layer& prev = p.lay[u.c[ci - 1]];
            RG_CALL(dgrad(p.lay[u.c[ci]], p.draw, p.draw3, nullptr, nullptr, x3 ? &prev : nullptr, ws.f(p.dt)));
            RG_CALL(bn_bwd(prev, ws.f(p.dt), true, nullptr, nullptr, p.draw, p.draw3));
            RG_CALL(wgrad(prev, p.draw, p.draw3));
        }
        RG_CALL(dgrad(p.lay[u.c[0]], p.draw, p.draw3, dskip, dskip_bits, x3 ? prev_last : nullptr, ws.f(p.g[cur ^ 1])));
        cur ^= 1;
    }

    // ---- stem tail: max-pool + BatchNorm/ReLU backward in one pass, then the input and weight gradients ----
    const float* sss = ws.f(p.stem_ss);
    const uint32_t* nz = (const uint32_t*)(ws.base + p.nz);
    uint8_t* tact = nullptr;
    if (!dx) {      // the weight gradient -- draw's only reader -- skips the tiles without a non-zero input under them
        tact = (uint8_t*)(ws.base + p.tact);
        RG_CALL(straps_stem_tile_activity(nz, tact, B, C, h, w, stream));
    }
    float* sdraw = ws.f(p.sdraw);
    RG_CALL(straps_bn_bwd_pooled_sparse(ws.f(p.g[cur]), (const uint8_t*)(ws.base + p.idx), ws.f(p.stem_raw), sss + 128, sss + 192, params + p.stem.gb_off,
                                        sss, sss + 64, dgamma(p.stem.gb_off), dbeta(p.stem.gb_off, 64), sdraw, bnws, B, p.geo.Hs, p.geo.Ws, 64, 0, tact, stream));
    if (dx) {
        RG_CALL(straps_pack_stem_dgrad_weight(params + p.stem.w_off, ws.f(p.wsd), C, stream));
        RG_CALL(straps_stem_dgrad(sdraw, ws.f(p.wsd), dx, B, C, h, w, 0, stream));
    }
    if (pg) RG_CALL(straps_stem_wgrad(x, sdraw, grads + p.stem.w_off, ws.base + p.swgws, nz, B, C, h, w, 0, stream));
    return STRAPS_OK;
}

extern "C" int straps_regressor_export_infer_params(const straps_regressor_desc_t* d, const float* params, const float* bn_state,
                                                    const float* init_est, float* infer_params, void* stream) {
    static const char* fn = "straps_regressor_export_infer_params";
    const char* bad = check_desc(d, true);
    STRAPS_REQUIRE(!bad, "%s: %s", fn, bad);
    STRAPS_REQUIRE(params, "%s: null pointer `params`", fn);
    STRAPS_REQUIRE(bn_state, "%s: null pointer `bn_state`", fn);
    STRAPS_REQUIRE(init_est, "%s: null pointer `init_est`", fn);
    STRAPS_REQUIRE(infer_params, "%s: null pointer `infer_params`", fn);
    Net n;
    make_net(d, n);
    hipStream_t st = (hipStream_t)stream;
    auto copy = [&](long long dst, const float* src, long long count) -> int {
        const hipError_t e = hipMemcpyAsync(infer_params + dst, src, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) {
            straps_set_error("%s: hipMemcpyAsync failed: %s", fn, hipGetErrorString(e));
            return STRAPS_EHIP;
        }
        return STRAPS_OK;
    };
    // per layer: weight, gamma + beta (adjacent in `params`), running mean + var (adjacent in `bn_state`)
    auto layer = [&](const Conv& cv) -> int {
        RG_CALL(copy(cv.inf_w, params + cv.w_off, cv.weights()));
        RG_CALL(copy(cv.inf_bn, params + cv.gb_off, 2LL * cv.cout));
        return copy(cv.inf_bn + 2LL * cv.cout, bn_state + cv.rs_off, 2LL * cv.cout);
    };
    RG_CALL(layer(n.stem));
    for (int i = 0; i < n.nconvs; ++i) RG_CALL(layer(n.convs[i]));
    RG_CALL(copy(n.ief_inf.fc1w, params + n.ief.fc1w, n.train_floats - n.ief.fc1w));      // the IEF tensors: the same order in both layouts
    RG_CALL(copy(n.inf_init, init_est, kNumParams));
    return STRAPS_OK;
}
