// regressor_net.h -- the network description the regressor C entry points share (regressor.hip: inference, regressor_train.hip:
// training).  One walk of the ResNet-18/50 encoder and the IEF head gives every layer's shape and its offsets in the three flat parameter
// layouts; one geometry function gives the stem / pool extents and every convolution's input and output extent for an input; the IEF
// forward and the argument checks both sides make are here once.
#pragma once

#include "common.h"

namespace {

constexpr int kEstLd = 160;           // IEF estimate row stride (ief_module.EST_LD): 157 padded to a multiple of 8
constexpr int kNumParams = 157;       // cam 3 | pose 24 x 6 | shape 10
constexpr float kBnEps = 1e-5f;       // nn.BatchNorm2d defaults (not part of the state dict)
constexpr float kBnMomentum = 0.1f;
constexpr size_t kAlign = 256;        // every region of the prepared buffer and the workspaces starts on this boundary
constexpr int kMaxConvs = 56;         // resnet50 has 52 convolutions besides the stem (the training workspace sizes its pack table from this)

size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }
long long round8(long long v) { return (v + 7) / 8 * 8; }
int conv_out(int h, int k, int s, int p) { return (h + 2 * p - k) / s + 1; }

#define RG_CALL(expr)                         \
    do {                                      \
        const int rc__ = (expr);              \
        if (rc__ != STRAPS_OK) return rc__;   \
    } while (0)

// nullptr + text when the description is invalid (the text names the field)
const char* check_desc(const straps_regressor_desc_t* d, bool training) {
    if (!d) return "null pointer `desc`";
    if (d->layers != 18 && d->layers != 50) return "`layers` must be 18 or 50";
    // (the stem keeps all input channels' weights in LDS: 256 channels fit its 160 KiB)
    if (d->in_channels < 1 || d->in_channels > 256) return "`in_channels` must be in [1, 256]";
    if (d->ief_iters < 1 || d->ief_iters > 64) return "`ief_iters` must be in [1, 64]";
    // (2 is unassigned: it stays invalid; 3 = bf16 is an inference-only route, no train entry point accepts it)
    if (training && d->precision != 0 && d->precision != 1)
        return "`precision` must be 0 (bf16x3) or 1 (fp32) for training (3 = bf16 is inference-only)";
    if (d->precision != 0 && d->precision != 1 && d->precision != 3) return "`precision` must be 0 (bf16x3), 1 (fp32) or 3 (bf16)";
    return nullptr;
}

// one convolution (the stem included) and its tensors' offsets (floats) in every layout
struct Conv {
    int cin, cout, k, stride, pad;
    bool relu, last;                  // ReLU after the BatchNorm (all but a projection); last convolution of a unit (adds the identity)
    long long first;                  // element offset in the packed weights (state-dict order = ResNet.prepack's; not the stem)
    long long inf_w, inf_bn;          // inference layout (state_dict()): OIHW weight; gamma, beta, running_mean, running_var
    long long w_off, gb_off;          // training layout (regressor.parameters()): OIHW weight; gamma then beta
    long long rs_off;                 // bn_state: running_mean then running_var
    long long weights() const { return (long long)cout * cin * k * k; }
};

struct Unit {
    int c[3], nconv;                  // indices into Net::convs
    bool has_ds;
    int ds;                           // the projection (state-dict order: after the unit's own convolutions)
};

struct Ief {
    long long fc1w, fc1b, fc2w, fc2b, fc3w, fc3b;
};

struct Net {
    int layers, cin, iters, precision;
    int F, H1, H2;
    Conv stem;
    Conv convs[kMaxConvs];            // non-stem convolutions in state-dict order
    int nconvs;
    Unit units[16];
    int nunits;
    long long conv_total, ps;         // sum of the non-stem weight elements; the plane stride of packed weight planes
    Ief ief, ief_inf;                 // the IEF tensors: the same order in both layouts
    long long inf_init;               // the inference layout ends with the initial estimate
    long long inf_floats, train_floats, bn_floats;
};

void make_net(const straps_regressor_desc_t* d, Net& n) {
    n.layers = d->layers;
    n.cin = d->in_channels;
    n.iters = d->ief_iters;
    n.precision = d->precision;
    const bool bottleneck = d->layers == 50;
    const int blocks18[4] = {2, 2, 2, 2}, blocks50[4] = {3, 4, 6, 3};
    const int* blocks = bottleneck ? blocks50 : blocks18;
    const int expansion = bottleneck ? 4 : 1;
    long long inf = 0, tr = 0, rs = 0, first = 0;
    auto place = [&](Conv& cv, int cin, int cout, int k, int stride, int pad, bool relu, bool last) {
        cv.cin = cin; cv.cout = cout; cv.k = k; cv.stride = stride; cv.pad = pad;
        cv.relu = relu; cv.last = last;
        const long long nw = cv.weights();
        cv.inf_w = inf; cv.inf_bn = inf + nw; inf += nw + 4LL * cout;
        cv.w_off = tr; cv.gb_off = tr + nw; tr += nw + 2LL * cout;
        cv.rs_off = rs; rs += 2LL * cout;
    };
    auto conv = [&](int cin, int cout, int k, int stride, int pad, bool relu, bool last) {
        Conv& cv = n.convs[n.nconvs];
        place(cv, cin, cout, k, stride, pad, relu, last);
        cv.first = first;
        first += cv.weights();
        return n.nconvs++;
    };
    n.nconvs = 0;
    n.nunits = 0;
    place(n.stem, n.cin, 64, 7, 2, 3, true, false);
    n.stem.first = 0;
    int inplanes = 64;
    for (int li = 0; li < 4; ++li) {
        const int planes = 64 << li, stride = li == 0 ? 1 : 2;
        for (int bi = 0; bi < blocks[li]; ++bi) {
            Unit& u = n.units[n.nunits++];
            const int s = bi == 0 ? stride : 1, outp = planes * expansion;
            // state-dict order of a unit: its own convolutions, then the projection (ResidualUnit registers `downsample` last)
            if (bottleneck) {
                u.nconv = 3;
                u.c[0] = conv(inplanes, planes, 1, 1, 0, true, false);
                u.c[1] = conv(planes, planes, 3, s, 1, true, false);
                u.c[2] = conv(planes, outp, 1, 1, 0, true, true);
            } else {
                u.nconv = 2;
                u.c[0] = conv(inplanes, planes, 3, s, 1, true, false);
                u.c[1] = conv(planes, planes, 3, 1, 1, true, true);
            }
            u.has_ds = bi == 0 && (s != 1 || inplanes != outp);
            u.ds = u.has_ds ? conv(inplanes, outp, 1, s, 0, false, false) : -1;
            inplanes = outp;
        }
    }
    n.conv_total = first;
    n.ps = round8(first);
    n.F = inplanes;
    n.H1 = n.H2 = bottleneck ? 1024 : 512;
    auto ief = [&](Ief& l, long long off) {
        l.fc1w = off; off += (long long)n.H1 * (n.F + kNumParams);
        l.fc1b = off; off += n.H1;
        l.fc2w = off; off += (long long)n.H2 * n.H1;
        l.fc2b = off; off += n.H2;
        l.fc3w = off; off += (long long)kNumParams * n.H2;
        l.fc3b = off; off += kNumParams;
        return off;
    };
    n.train_floats = ief(n.ief, tr);
    n.inf_init = ief(n.ief_inf, inf);
    n.inf_floats = n.inf_init + kNumParams;
    n.bn_floats = rs;
}

struct Extent {
    int H, W, Ho, Wo;                 // input / output extent of one convolution
};

struct Geometry {
    int Hs, Ws, Hp, Wp, Hf, Wf;       // stem output, pooled, encoder output
    Extent e[kMaxConvs];              // in Net::convs order
};

// the extents for one (batch, h, w); false if the input is too small for the network
bool make_geometry(const Net& n, int B, int H, int W, Geometry& g) {
    if (B <= 0 || H < 7 || W < 7) return false;
    g.Hs = conv_out(H, 7, 2, 3); g.Ws = conv_out(W, 7, 2, 3);
    g.Hp = conv_out(g.Hs, 3, 2, 1); g.Wp = conv_out(g.Ws, 3, 2, 1);
    int h = g.Hp, w = g.Wp;
    auto extent = [&](int i, int ih, int iw) {
        const Conv& cv = n.convs[i];
        Extent& e = g.e[i];
        e.H = ih; e.W = iw;
        e.Ho = conv_out(ih, cv.k, cv.stride, cv.pad); e.Wo = conv_out(iw, cv.k, cv.stride, cv.pad);
        return e.Ho > 0 && e.Wo > 0;
    };
    for (int ui = 0; ui < n.nunits; ++ui) {
        const Unit& u = n.units[ui];
        if (u.has_ds && !extent(u.ds, h, w)) return false;
        for (int ci = 0; ci < u.nconv; ++ci) {
            if (!extent(u.c[ci], h, w)) return false;
            h = g.e[u.c[ci]].Ho;
            w = g.e[u.c[ci]].Wo;
        }
    }
    g.Hf = h; g.Wf = w;
    return true;
}

// the argument checks both forwards and the backward share
int check_args(const char* fn, const straps_regressor_desc_t* d, bool training, const float* x, int batch, int h, int w, const void* workspace) {
    const char* bad = check_desc(d, training);
    STRAPS_REQUIRE(!bad, "%s: %s", fn, bad);
    STRAPS_REQUIRE(x, "%s: null pointer `x`", fn);
    STRAPS_REQUIRE(workspace, "%s: null pointer `workspace`", fn);
    STRAPS_REQUIRE(batch >= 1, "%s: `batch` must be positive (got %d)", fn, batch);
    STRAPS_REQUIRE(h >= 7 && w >= 7, "%s: `h` and `w` must be at least 7 (got %d x %d)", fn, h, w);
    STRAPS_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, "%s: `workspace` must be %zu-byte aligned", fn, kAlign);
    STRAPS_REQUIRE(((uintptr_t)x & 3) == 0, "%s: `x` must be float-aligned", fn);
    return STRAPS_OK;
}

// global average pool of the encoder output `enc` [B][hw][F], then the IEF iterations (IEFModule.forward_estimate).  ests [T + 1][B][160]
// starts as copies of `init`; iteration it reads slot it, writes slot it + 1 and keeps its hidden activations at h1 + it * h1_step,
// h2 + it * h2_step (step 0: one pair, overwritten).  w1f / w1e / w3: the straps_ief_pack views of fc1 / fc3.
int ief_forward(const Net& n, int B, const float* enc, int hw, const float* init, const float* w1f, const float* w1e, const float* fc1b,
                const float* fc2w, const float* fc2b, const float* w3, const float* fc3b, float* feat, float* c1, float* ests, float* h1,
                long long h1_step, float* h2, long long h2_step, float* est, int ld_est, void* stream) {
    const int F = n.F, H1 = n.H1, H2 = n.H2, T = n.iters;
    RG_CALL(straps_gap_fwd(enc, feat, B, hw, F, stream));
    RG_CALL(straps_broadcast_rows(init, kNumParams, ests, kEstLd, (T + 1) * B, stream));
    RG_CALL(straps_linear_fwd(feat, F, w1f, F, fc1b, nullptr, c1, H1, B, H1, F, 0, stream));
    // with ld_est == 160 the last iteration writes `est` itself (the fc3 epilogue reads its addend with the output's row stride);
    // otherwise it writes the last slot, copied out below
    const bool direct = ld_est == kEstLd;
    for (int it = 0; it < T; ++it) {
        float* est_in = ests + (size_t)it * B * kEstLd;
        float* est_out = direct && it == T - 1 ? est : est_in + (size_t)B * kEstLd;
        float* h1i = h1 + it * h1_step;
        float* h2i = h2 + it * h2_step;
        RG_CALL(straps_linear_fwd(est_in, kEstLd, w1e, kEstLd, nullptr, c1, h1i, H1, B, H1, kEstLd, 1, stream));
        RG_CALL(straps_linear_fwd(h1i, H1, fc2w, H1, fc2b, nullptr, h2i, H2, B, H2, H1, 1, stream));
        RG_CALL(straps_linear_fwd(h2i, H2, w3, H2, fc3b, est_in, est_out, kEstLd, B, kNumParams, H2, 0, stream));
    }
    if (!direct) RG_CALL(straps_masked_copy(ests + (size_t)T * B * kEstLd, kEstLd, nullptr, 0, est, ld_est, B, kNumParams, 0, stream));
    return STRAPS_OK;
}

}  // namespace
