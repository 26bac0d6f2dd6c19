// C-ABI of the skinny weight-gradient product (lora_wgrad.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/visualrwkv_hip.h"
#include <host_checks.h>
#include <lora_wgrad.h>
#include <wgrad_big.h>
#include <patch_wgrad.h>

using hostchk::any_misaligned, hostchk::any_null, hostchk::finish_launch, hostchk::launch_lds;

namespace {

// M-slices: ~2 workgroups per CU of the 256; more slices cost more partial-sum traffic than they hide latency
int splits(long M, int Nw, int D) {
    const long nsteps = (M + lwg::KS - 1) / lwg::KS;
    long s = (D <= 160 ? 512 : 256) / (Nw / lwg::CT);     // measured at Nw = 2048: 32 slices (16 for D = 256, which runs
                                                          // two column groups per slice) beat 24, 48 and 64
    if (s < 1) s = 1;
    return (int)(s < nsteps ? s : nsteps);
}
bool supported_d(int D) { return D == 32 || D == 64 || D == 96 || D == 128 || D == 160 || D == 256; }

template <int ND>
int launch(const lwg::Args& a, int S, hipStream_t st) {
    constexpr int D = 16 * ND;                           // Narrow columns per workgroup; a.D / D column groups
    const size_t lds = 2 * lwg::KS * (size_t)(lwg::WS + D + 8) * sizeof(uint16_t);
    hipLaunchKernelGGL((lwg::wgrad_kernel<ND>), dim3((unsigned)(a.Nw / lwg::CT * (a.D / D)), (unsigned)S), dim3(256), lds, st, a);
    return finish_launch();
}

}  // namespace

extern "C" long vrwkv_wgrad_skinny_ws_floats(long M, int Nw, int D) {
    if (M <= 0 || Nw <= 0 || Nw % lwg::CT != 0 || !supported_d(D)) return -1;
    return (long)splits(M, Nw, D) * Nw * D;
}

extern "C" int vrwkv_wgrad_skinny_bf16(long M, int Nw, int D, const void* wide, const void* narrow, void* out, int transposed,
                                       float* ws, void* stream) {
    if (M <= 0 || any_null(wide, narrow, out, ws)) return VRWKV_EINVAL;
    if (Nw <= 0 || Nw % lwg::CT != 0 || !supported_d(D)) return VRWKV_ESHAPE;
    if (any_misaligned(wide, narrow, ws)) return VRWKV_EALIGN;      // not out
    const hipStream_t st = (hipStream_t)stream;
    const int S = splits(M, Nw, D);
    const lwg::Args a{M, Nw, D, (const uint16_t*)wide, (const uint16_t*)narrow, ws};
    int e = 0;
    switch (D / 16) {
        case 2: e = launch<2>(a, S, st); break;
        case 4: e = launch<4>(a, S, st); break;
        case 6: e = launch<6>(a, S, st); break;
        case 8: e = launch<8>(a, S, st); break;
        case 10: e = launch<10>(a, S, st); break;
        default: e = launch<8>(a, S, st); break;      // D = 256: two column groups of 128
    }
    if (e) return e;
    const long n = (long)Nw * D;
    hipLaunchKernelGGL(lwg::reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, ws, S, Nw, D, transposed, (uint16_t*)out);
    return finish_launch();
}

// ---- the square / wide weight gradients (wgrad_big.h): C (N1 x N2) = A^T B, A (M x N1), B (M x N2)
namespace {
// M-slices so that the grid has at least one workgroup per CU (256): the C x C shapes have 64 tiles -> 4 slices
int big_splits(long M, int N1, int N2) {
    const long tiles = (long)(N1 / wgb::TM) * (N2 / wgb::TN);
    long s = (256 + tiles - 1) / tiles;
    const long nst = M / wgb::KT;
    if (s > 8) s = 8;
    return (int)(s < 1 ? 1 : (s < nst ? s : nst));
}
// sums the S partial products of ws (n floats each) into the bf16 out
void launch_big_reduce(float* ws, int S, long n, void* out, hipStream_t st) {
    const long blocks = (n / 4 + 255) / 256;
    hipLaunchKernelGGL(wgb::wgrad_big_reduce, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, st, ws, S, n, (uint16_t*)out);
}
}  // namespace

extern "C" long vrwkv_wgrad_big_ws_floats(long M, int N1, int N2) {
    if (M <= 0 || M % wgb::KT != 0 || N1 <= 0 || N2 <= 0 || N1 % wgb::TM != 0 || N2 % wgb::TN != 0) return -1;
    const int S = big_splits(M, N1, N2);
    return S > 1 ? (long)S * N1 * N2 : 0;
}

extern "C" int vrwkv_wgrad_big_bf16(long M, int N1, int N2, const void* A, const void* B, void* out, float* ws, void* stream) {
    if (M <= 0 || any_null(A, B, out)) return VRWKV_EINVAL;
    if (M % wgb::KT != 0 || N1 <= 0 || N2 <= 0 || N1 % wgb::TM != 0 || N2 % wgb::TN != 0) return VRWKV_ESHAPE;
    if (any_misaligned(A, B, out, ws)) return VRWKV_EALIGN;          // ws may be NULL
    const int S = big_splits(M, N1, N2);
    if (S > 1 && !ws) return VRWKV_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    const wgb::Args a{M, N1, N2, S, (const uint16_t*)A, (const uint16_t*)B, ws, (uint16_t*)out};
    const size_t lds = (size_t)wgb::STAGES * 2 * wgb::OPB;
    if (int rc = launch_lds(&wgb::wgrad_big_kernel, dim3((unsigned)((N1 / wgb::TM) * (N2 / wgb::TN) * S)), dim3(512), lds, st, a)) return rc;
    if (S > 1) launch_big_reduce(ws, S, (long)N1 * N2, out, st);
    return finish_launch();
}

// ---- weight gradient of a trained patch embedding (patch_wgrad.h): dW (N x 768) = dout^T patches(pixels), dbias = column sums
namespace {
constexpr int PATCH_P = 16, PATCH_K = 3 * PATCH_P * PATCH_P;       // 768 = three tile columns, one per colour channel
constexpr int BIAS_SLICES = 64;                                    // row slices of the dbias partial sums
inline int bias_slices(long M) { return (int)(M / wgb::KT < BIAS_SLICES ? M / wgb::KT : BIAS_SLICES); }
inline bool patch_shape_ok(int B, int Himg, int Wimg, int P, int N) {
    if (B <= 0 || Himg <= 0 || Wimg <= 0 || N <= 0) return false;
    if (P != PATCH_P || Himg % PATCH_P != 0 || Wimg % PATCH_P != 0 || N % wgb::TM != 0) return false;
    const long M = (long)B * (Himg / PATCH_P) * (Wimg / PATCH_P);
    if (M % wgb::KT != 0 || M >= (1L << 31)) return false;
    return (long)B * 3 * Himg * Wimg * 2 < (1L << 32);             // the kernel's pixel byte offsets are 32-bit
}
}  // namespace

extern "C" long vrwkv_patch_embed_wgrad_ws_floats(int B, int Himg, int Wimg, int P, int N) {
    if (!patch_shape_ok(B, Himg, Wimg, P, N)) return -1;
    const long M = (long)B * (Himg / PATCH_P) * (Wimg / PATCH_P);
    const int S = big_splits(M, N, PATCH_K);
    return (S > 1 ? (long)S * N * PATCH_K : 0) + (long)bias_slices(M) * N;
}

extern "C" int vrwkv_patch_embed_wgrad_bf16(int B, int Himg, int Wimg, int P, int N, const void* pixels, const void* dout, void* dW,
                                            void* dbias, float* ws, void* stream) {
    if (B <= 0 || Himg <= 0 || Wimg <= 0 || N <= 0 || any_null(pixels, dout, dW, ws)) return VRWKV_EINVAL;
    if (!patch_shape_ok(B, Himg, Wimg, P, N)) return VRWKV_ESHAPE;
    if (any_misaligned(pixels, dout, dW, ws)) return VRWKV_EALIGN;
    const int gw = Wimg / PATCH_P, Mimg = (Himg / PATCH_P) * gw;
    const long M = (long)B * Mimg;
    const int S = big_splits(M, N, PATCH_K);
    const hipStream_t st = (hipStream_t)stream;
    const wgp::Args a{M, N, PATCH_K, S, (const uint16_t*)dout, (const uint16_t*)pixels, ws, (uint16_t*)dW, Mimg, gw, Himg, Wimg,
                      wgp::Div::make((unsigned)Mimg), wgp::Div::make((unsigned)gw)};
    const size_t lds = (size_t)wgb::STAGES * 2 * wgb::OPB;
    if (int rc = launch_lds(&wgp::wgrad_patch_kernel, dim3((unsigned)((N / wgb::TM) * 3 * S)), dim3(512), lds, st, a)) return rc;
    const long n = (long)N * PATCH_K;
    if (S > 1) {
        launch_big_reduce(ws, S, n, dW, st);
        if (int rc = finish_launch()) return rc;
    }
    if (dbias) {
        float* part = ws + (S > 1 ? (size_t)S * n : 0);
        const int G = bias_slices(M);
        hipLaunchKernelGGL(wgp::colsum_part_kernel, dim3((unsigned)(N / 256), (unsigned)G), dim3(256), 0, st, M, N, (const uint16_t*)dout, part);
        hipLaunchKernelGGL(wgp::colsum_finish_kernel, dim3((unsigned)(N / 256)), dim3(256), 0, st, G, N, part, (uint16_t*)dbias);
    }
    return finish_launch();
}
