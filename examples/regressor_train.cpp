// regressor_train.cpp -- a few SingleInputRegressor training steps from C++ without torch: include/straps_hip.h, the HIP runtime and
// libstraps_hip.so.  Per step: straps_regressor_fwd_train, a mean squared error to a fixed target estimate (on the host),
// straps_regressor_bwd into the flat gradient buffer, straps_adam_step over the flat parameter buffer.
//
// Build (from the repository root, after the library is built):
//   hipcc --offload-arch=gfx950 -I include examples/regressor_train.cpp -o regressor_train \
//         -L straps-3dhumanshapepose_amd/csrc -lstraps_hip -Wl,-rpath,$PWD/straps-3dhumanshapepose_amd/csrc
//
// Run:
//   regressor_train <layers 18|50> <in_channels> <ief_iters> <precision 0=bf16x3|1=fp32> <batch> <h> <w> <steps>
//                   <params.bin> <bn_state.bin> <init_est.bin>
//
// params.bin: straps_regressor_train_param_floats() fp32 values (train_abi.flat_training_params writes them from a module);
// bn_state.bin: straps_regressor_bn_state_floats() values (train_abi.flat_bn_state); init_est.bin: the IEF's 157-float initial
// estimate.  The input batch is synthetic and fixed: a sparse pattern like the proxy representation's.  Prints one loss per step;
// exits non-zero, with the library's message, on any failure.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "straps_hip.h"

static void die(const char* what, const char* why) {
    std::fprintf(stderr, "regressor_train: %s: %s\n", what, why);
    std::exit(1);
}

#define HIP_OK(expr)                                              \
    do {                                                          \
        hipError_t e_ = (expr);                                   \
        if (e_ != hipSuccess) die(#expr, hipGetErrorString(e_));  \
    } while (0)

#define STRAPS_OK_OR_DIE(expr)                                    \
    do {                                                          \
        if ((expr) != STRAPS_OK) die(#expr, straps_last_error()); \
    } while (0)

static std::vector<float> read_floats(const std::string& path, size_t n) {
    std::vector<float> v(n);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) die(path.c_str(), "cannot open");
    const size_t got = std::fread(v.data(), sizeof(float), n, f);
    const bool extra = std::fgetc(f) != EOF;
    std::fclose(f);
    if (got != n || extra) die(path.c_str(), "wrong size");
    return v;
}

int main(int argc, char** argv) {
    if (argc != 12) {
        std::fprintf(stderr, "usage: %s layers in_channels ief_iters precision batch h w steps params.bin bn_state.bin init_est.bin\n", argv[0]);
        return 2;
    }
    straps_regressor_desc_t desc;
    desc.layers = std::atoi(argv[1]);
    desc.in_channels = std::atoi(argv[2]);
    desc.ief_iters = std::atoi(argv[3]);
    desc.precision = std::atoi(argv[4]);
    const int batch = std::atoi(argv[5]), h = std::atoi(argv[6]), w = std::atoi(argv[7]), steps = std::atoi(argv[8]);
    const int P = 157, ld = 160;

    const size_t n_params = straps_regressor_train_param_floats(&desc);
    const size_t n_bn = straps_regressor_bn_state_floats(&desc);
    const size_t ws_bytes = straps_regressor_train_workspace_bytes(&desc, batch, h, w);
    if (!n_params || !n_bn) die("regressor description", "invalid (layers 18|50, in_channels 1..256, ief_iters >= 1, precision 0|1)");
    if (!ws_bytes) die("input geometry", "invalid (batch >= 1, h and w >= 7)");
    if (steps < 1) die("steps", "must be positive");
    const std::vector<float> params = read_floats(argv[9], n_params);
    const std::vector<float> bn_state = read_floats(argv[10], n_bn);
    const std::vector<float> init_est = read_floats(argv[11], P);

    // the fixed batch: about 2 % non-zero cells, and a target estimate near the initial one
    std::vector<float> input((size_t)batch * desc.in_channels * h * w, 0.f);
    unsigned s = 12345u;
    for (float& v : input) {
        s = s * 1664525u + 1013904223u;
        if ((s >> 8) % 50 == 0) v = (float)((s >> 16) & 0xff) / 255.f;
    }
    std::vector<float> target((size_t)batch * P);
    for (int b = 0; b < batch; ++b)
        for (int j = 0; j < P; ++j) target[(size_t)b * P + j] = init_est[j] + 0.1f * std::sin(0.37f * j + 1.3f * b);

    float *d_params, *d_bn, *d_init, *d_x, *d_est, *d_dest, *d_grads, *d_m, *d_v;
    void* d_ws;
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));
    HIP_OK(hipMalloc(&d_params, n_params * sizeof(float)));
    HIP_OK(hipMalloc(&d_grads, n_params * sizeof(float)));
    HIP_OK(hipMalloc(&d_m, n_params * sizeof(float)));
    HIP_OK(hipMalloc(&d_v, n_params * sizeof(float)));
    HIP_OK(hipMalloc(&d_bn, n_bn * sizeof(float)));
    HIP_OK(hipMalloc(&d_init, P * sizeof(float)));
    HIP_OK(hipMalloc(&d_x, input.size() * sizeof(float)));
    HIP_OK(hipMalloc(&d_est, (size_t)batch * ld * sizeof(float)));
    HIP_OK(hipMalloc(&d_dest, (size_t)batch * ld * sizeof(float)));
    HIP_OK(hipMalloc(&d_ws, ws_bytes));
    HIP_OK(hipMemcpy(d_params, params.data(), n_params * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_bn, bn_state.data(), n_bn * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_init, init_est.data(), P * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_x, input.data(), input.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_m, 0, n_params * sizeof(float)));      // Adam's moments start at zero
    HIP_OK(hipMemset(d_v, 0, n_params * sizeof(float)));

    std::vector<float> est((size_t)batch * ld), dest((size_t)batch * ld, 0.f);
    const double scale = 1.0 / ((double)batch * P);
    for (int step = 1; step <= steps; ++step) {
        STRAPS_OK_OR_DIE(straps_regressor_fwd_train(&desc, d_params, d_bn, d_init, d_x, batch, h, w, d_est, ld, d_ws, ws_bytes, stream));
        HIP_OK(hipMemcpyAsync(est.data(), d_est, est.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        // loss = mean (est - target)^2 over the 157 columns; dest = its gradient
        double loss = 0.0;
        for (int b = 0; b < batch; ++b)
            for (int j = 0; j < P; ++j) {
                const double r = (double)est[(size_t)b * ld + j] - target[(size_t)b * P + j];
                loss += r * r * scale;
                dest[(size_t)b * ld + j] = (float)(2.0 * r * scale);
            }
        std::printf("step %d loss %.9g\n", step, loss);
        HIP_OK(hipMemcpyAsync(d_dest, dest.data(), dest.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        STRAPS_OK_OR_DIE(straps_regressor_bwd(&desc, d_params, d_x, batch, h, w, d_dest, ld, d_grads, nullptr, d_ws, ws_bytes, stream));
        STRAPS_OK_OR_DIE(straps_adam_step(d_params, d_grads, d_m, d_v, (long long)n_params, step, 1e-4f, 0.9f, 0.999f, 1e-8f, 1.0f, nullptr, stream));
    }
    HIP_OK(hipStreamSynchronize(stream));
    std::printf("regressor_train: resnet%d, %d x %d x %d x %d, %d steps; %zu parameters, workspace %.1f MB\n", desc.layers, batch,
                desc.in_channels, h, w, steps, n_params, ws_bytes / 1048576.0);
    for (void* p : {(void*)d_params, (void*)d_grads, (void*)d_m, (void*)d_v, (void*)d_bn, (void*)d_init, (void*)d_x, (void*)d_est, (void*)d_dest, d_ws})
        HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(stream));
    return 0;
}
