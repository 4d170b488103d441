// regressor_infer.cpp -- SingleInputRegressor inference from C++ without torch: include/straps_hip.h, the HIP runtime and libstraps_hip.so.
//
// Build (from the repository root, after the library is built):
//   hipcc --offload-arch=gfx950 -I include examples/regressor_infer.cpp -o regressor_infer \
//         -L straps-3dhumanshapepose_amd/csrc -lstraps_hip -Wl,-rpath,$PWD/straps-3dhumanshapepose_amd/csrc
//
// Run:
//   regressor_infer <layers 18|50> <in_channels> <ief_iters> <precision 0=bf16x3|1=fp32> <batch> <h> <w> <params.bin> <input.bin> <out_dir>
//
// params.bin: straps_regressor_param_floats() fp32 values in the layout of straps_hip.h (infer.flat_inference_params writes it from a
// module); input.bin: batch * in_channels * h * w fp32 values, NCHW.  Writes <out_dir>/est.bin ([batch][157]: cam 3 | pose 144 | shape 10)
// and <out_dir>/rotmats.bin ([batch][24][3][3]).  Exits non-zero, with the library's message, on any failure.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "straps_hip.h"

static void die(const char* what, const char* why) {
    std::fprintf(stderr, "regressor_infer: %s: %s\n", what, why);
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

static void write_floats(const std::string& path, const std::vector<float>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) die(path.c_str(), "cannot create");
    const size_t put = std::fwrite(v.data(), sizeof(float), v.size(), f);
    if (std::fclose(f) != 0 || put != v.size()) die(path.c_str(), "write failed");
}

int main(int argc, char** argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: %s layers in_channels ief_iters precision batch h w params.bin input.bin out_dir\n", argv[0]);
        return 2;
    }
    straps_regressor_desc_t desc;
    desc.layers = std::atoi(argv[1]);
    desc.in_channels = std::atoi(argv[2]);
    desc.ief_iters = std::atoi(argv[3]);
    desc.precision = std::atoi(argv[4]);
    const int batch = std::atoi(argv[5]), h = std::atoi(argv[6]), w = std::atoi(argv[7]);
    const std::string out_dir = argv[10];

    const size_t n_params = straps_regressor_param_floats(&desc);
    const size_t prepared_bytes = straps_regressor_prepared_bytes(&desc);
    const size_t ws_bytes = straps_regressor_workspace_bytes(&desc, batch, h, w);
    if (!n_params || !prepared_bytes) die("regressor description", "invalid (layers 18|50, in_channels 1..256, ief_iters >= 1, precision 0|1)");
    if (!ws_bytes) die("input geometry", "invalid (batch >= 1, h and w >= 7)");
    const std::vector<float> params = read_floats(argv[8], n_params);
    const std::vector<float> input = read_floats(argv[9], (size_t)batch * desc.in_channels * h * w);

    const int ld_est = 157;
    float *d_params = nullptr, *d_x = nullptr, *d_est = nullptr, *d_rot = nullptr;
    void *d_prepared = nullptr, *d_ws = nullptr;
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));
    HIP_OK(hipMalloc(&d_params, n_params * sizeof(float)));
    HIP_OK(hipMalloc(&d_prepared, prepared_bytes));
    HIP_OK(hipMalloc(&d_x, input.size() * sizeof(float)));
    HIP_OK(hipMalloc(&d_est, (size_t)batch * ld_est * sizeof(float)));
    HIP_OK(hipMalloc(&d_rot, (size_t)batch * 24 * 9 * sizeof(float)));
    HIP_OK(hipMalloc(&d_ws, ws_bytes));
    HIP_OK(hipMemcpy(d_params, params.data(), n_params * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_x, input.data(), input.size() * sizeof(float), hipMemcpyHostToDevice));

    // one-time: fold BatchNorm, pack the weights (synchronises the stream); the parameter buffer is not read again
    STRAPS_OK_OR_DIE(straps_regressor_prepare(&desc, d_params, d_prepared, stream));
    HIP_OK(hipFree(d_params));
    STRAPS_OK_OR_DIE(straps_regressor_fwd_infer(&desc, d_prepared, d_x, batch, h, w, d_est, ld_est, d_rot, d_ws, ws_bytes, stream));
    HIP_OK(hipStreamSynchronize(stream));

    std::vector<float> est((size_t)batch * ld_est), rot((size_t)batch * 24 * 9);
    HIP_OK(hipMemcpy(est.data(), d_est, est.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rot.data(), d_rot, rot.size() * sizeof(float), hipMemcpyDeviceToHost));
    write_floats(out_dir + "/est.bin", est);
    write_floats(out_dir + "/rotmats.bin", rot);
    std::printf("regressor_infer: resnet%d, %d x %d x %d x %d -> est [%d][157], rotmats [%d][24][3][3]; workspace %.1f MB, prepared %.1f MB\n",
                desc.layers, batch, desc.in_channels, h, w, batch, batch, ws_bytes / 1048576.0, prepared_bytes / 1048576.0);
    HIP_OK(hipFree(d_prepared));
    HIP_OK(hipFree(d_x));
    HIP_OK(hipFree(d_est));
    HIP_OK(hipFree(d_rot));
    HIP_OK(hipFree(d_ws));
    HIP_OK(hipStreamDestroy(stream));
    return 0;
}
