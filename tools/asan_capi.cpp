// Host-side sanitizer pass over the C ABI: a small driver, built - like the library it links
// (mixq_amd/libmixq_hip_asan.so: the product sources with -fsanitize=address -fno-gpu-sanitize) - with AddressSanitizer on the HOST
// code.  The Python layer hands raw addresses across this boundary; nothing else checks the C side's host code (argument validation,
// the plan / workspace / per-device tables, launch-geometry arithmetic) for out-of-bounds accesses or use-after-free.
// What it walks: identification, every quantise / detect / dequant / re-tile entry point incl. empty inputs and rejected arguments, the
// kept-outlier-map routes, the fused GEMMs on every operand layout, mixq_linear_forward on a KEPT argument block (re-used, then edited),
// the RMSNorm entry points (the bfloat16 ones on their refusal and M == 0 paths, which need no device: that part also runs on a machine
// without a GPU, where the driver then stops; likewise the bfloat16 joint gate / up entry points of ABI 1.5), the W8A16 pair and its addend form - each followed by a device synchronise, results
// cross-checked where a second route exists.
//   build + run: tools/asan_capi.sh (on the GPU box)            exit code 0 and no ASAN report = clean
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/mixq_hip.h"

extern "C" int mixq_gemm_amax_supported(int, int, int, int);

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)
#define HIPOK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); exit(2); } } while (0)

template <class T> struct Dev {
    T* p = nullptr; size_t n = 0;
    explicit Dev(size_t n_) : n(n_) { HIPOK(hipMalloc(reinterpret_cast<void**>(&p), (n ? n : 1) * sizeof(T))); HIPOK(hipMemset(p, 0, (n ? n : 1) * sizeof(T))); }
    ~Dev() { (void)hipFree(p); }
    void up(const std::vector<T>& h) { HIPOK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
    std::vector<T> down() const { std::vector<T> h(n); HIPOK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost)); return h; }
};

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static uint16_t f2h(float f) { _Float16 h = static_cast<_Float16>(f); uint16_t b; memcpy(&b, &h, 2); return b; }
static float h2f(uint16_t b) { _Float16 h; memcpy(&h, &b, 2); return static_cast<float>(h); }

// the kept outlier map of include/mixq_hip.h (mixq_quant_fused_masked) for the first n entries of ind
static std::vector<uint32_t> kept_map(const std::vector<int32_t>& ind, int n, int K) {
    const int W = (K + 31) / 32, head = (W + 1 + 3) / 4 * 4;
    std::vector<uint32_t> m(head + (K + 7) / 8 * 4, 0u);
    std::vector<uint16_t> pos((K + 7) / 8 * 8, 0xffffu);                       // per-column AND-masks: 0 for an outlier column
    for (int j = 0; j < n; ++j) { m[ind[j] >> 5] |= 1u << (ind[j] & 31); pos[ind[j]] = 0; }
    m[W] = static_cast<uint32_t>(n);
    memcpy(m.data() + head, pos.data(), pos.size() * 2);
    return m;
}

// The bfloat16 RMSNorm entry points on the paths that end before any launch (refusals, M == 0): host code only, so this part also runs
// on a machine without a GPU.  The pointers are never dereferenced.
static void norm_bf16_host_paths() {
    uint16_t* p = reinterpret_cast<uint16_t*>(uintptr_t(4096));
    int32_t* pi = reinterpret_cast<int32_t*>(uintptr_t(4096));
    uint32_t* pm = reinterpret_cast<uint32_t*>(uintptr_t(4096));
    uint32_t* pm_odd = reinterpret_cast<uint32_t*>(uintptr_t(4096 + 8));
    const int K = 128, words = mixq_kept_map_words(K);
    CHECK(mixq_rmsnorm_bf16(nullptr, p, p, 4, K, K, K, 1e-5f, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_rmsnorm_bf16(p, nullptr, p, 4, K, K, K, 1e-5f, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_rmsnorm_bf16(p, p, nullptr, 4, K, K, K, 1e-5f, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_rmsnorm_bf16(p, p, p, 4, 132, 136, 136, 1e-5f, nullptr) == MIXQ_ESHAPE);           // K % 8
    CHECK(mixq_rmsnorm_bf16(p, p, p, 4, K, K, K - 8, 1e-5f, nullptr) == MIXQ_ESHAPE);             // ldout < K
    CHECK(mixq_rmsnorm_bf16(p, p, p, 4, 32776, 32776, 32776, 1e-5f, nullptr) == MIXQ_ESHAPE);     // more than 16 chunks per thread
    CHECK(mixq_rmsnorm_bf16(p, p, p, 0, K, K, K, 1e-5f, nullptr) == MIXQ_OK);
    CHECK(mixq_rmsnorm_bf16(nullptr, nullptr, nullptr, 0, K, K, K, 1e-5f, nullptr) == MIXQ_OK);   // empty inputs may carry null pointers
    for (int masked = 0; masked < 2; ++masked) {
        auto f = [&](const uint16_t* x, void* q, const int32_t* ind, int n, uint16_t* xo, int ldxo, int M, int Kv, int bit, int fmt, const uint32_t* map, int mw) {
            return masked ? mixq_rmsnorm_quant_fused_masked_bf16(x, p, p, ind, n, nullptr, map, mw, p, q, xo, nullptr, M, Kv, Kv, Kv, ldxo, 1e-5f, bit, 6.f, fmt, nullptr)
                          : mixq_rmsnorm_quant_fused_bf16(x, p, p, ind, n, nullptr, p, q, xo, nullptr, M, Kv, Kv, Kv, ldxo, 1e-5f, bit, 6.f, fmt, nullptr);
        };
        CHECK(f(nullptr, p, nullptr, 0, nullptr, 0, 4, K, 8, MIXQ_FMT_PLAIN, nullptr, 0) == MIXQ_EINVAL);
        CHECK(f(p, nullptr, nullptr, 0, nullptr, 0, 4, K, 8, MIXQ_FMT_PLAIN, nullptr, 0) == MIXQ_EINVAL);
        CHECK(f(p, p, nullptr, 0, nullptr, 0, 4, K, 5, MIXQ_FMT_PLAIN, nullptr, 0) == MIXQ_EINVAL);              // bit
        CHECK(f(p, p, nullptr, 0, nullptr, 0, 4, K, 8, MIXQ_FMT_F6X128, nullptr, 0) == MIXQ_EINVAL);             // FP6 codes are 4-bit
        CHECK(f(p, p, nullptr, 0, nullptr, 0, 4, 132, 8, MIXQ_FMT_PLAIN, nullptr, 0) == MIXQ_ESHAPE);            // K % 8
        CHECK(f(p, p, nullptr, 0, nullptr, 0, 4, 96, 8, MIXQ_FMT_P16X64, nullptr, 0) == MIXQ_ESHAPE);            // packed: K % 64
        CHECK(f(p, p, nullptr, 0, nullptr, 0, 4, 192, 4, MIXQ_FMT_R6X128, nullptr, 0) == MIXQ_ESHAPE);           // 4-bit packed: K / 2 % 64
        CHECK(f(p, p, nullptr, 0, nullptr, 0, 4, 32776, 8, MIXQ_FMT_PLAIN, nullptr, 0) == MIXQ_ESHAPE);
        CHECK(f(p, p, pi, 3, nullptr, 16, 4, K, 8, MIXQ_FMT_PLAIN, pm, words) == MIXQ_EINVAL);                   // n > 0 needs x_out
        CHECK(f(p, p, pi, 3, p, 2, 4, K, 8, MIXQ_FMT_PLAIN, pm, words) == MIXQ_EINVAL);                          // ldxo < n
        if (masked) {
            CHECK(f(p, p, pi, 3, p, 16, 4, K, 8, MIXQ_FMT_PLAIN, nullptr, words) == MIXQ_EINVAL);                // no map
            CHECK(f(p, p, pi, 3, p, 16, 4, K, 8, MIXQ_FMT_PLAIN, pm, words - 1) == MIXQ_EINVAL);                 // a shorter layout
            CHECK(f(p, p, pi, 3, p, 16, 4, K, 8, MIXQ_FMT_PLAIN, pm_odd, words) == MIXQ_EINVAL);                 // not 16-byte aligned
        }
        CHECK(f(p, p, pi, 3, p, 16, 0, K, 8, MIXQ_FMT_P16X64, pm, words) == MIXQ_OK);                            // M == 0: every check, no launch
        CHECK(f(p, p, nullptr, 0, nullptr, 0, 0, 256, 4, MIXQ_FMT_F6X128, nullptr, 0) == MIXQ_OK);
        CHECK(f(nullptr, nullptr, nullptr, 0, nullptr, 0, 0, K, 8, MIXQ_FMT_PLAIN, nullptr, 0) == MIXQ_OK);
    }
}

// The joint gate / up launch in bfloat16 (ABI 1.5) on the paths that end before any launch: every refusal of include/mixq_hip.h's list,
// M == 0, the query, and a forced tiling with and without the paired bf16 form.  Host code only; the pointers are never dereferenced.
static void pair_bf16_host_paths() {
    int8_t* q = reinterpret_cast<int8_t*>(uintptr_t(4096));
    uint8_t* q4 = reinterpret_cast<uint8_t*>(uintptr_t(4096));
    uint16_t* p = reinterpret_cast<uint16_t*>(uintptr_t(4096));
    uint16_t* p8 = reinterpret_cast<uint16_t*>(uintptr_t(4096 + 8));
    uint32_t* pm = reinterpret_cast<uint32_t*>(uintptr_t(4096));
    const int wf16 = MIXQ_X_PACKED | MIXQ_W_F16X64, f6 = MIXQ_XW_F6X128, M = 64, N = 128, K = 128;
    auto i8 = [&](const int8_t* qx, uint16_t* y, int ldy, int Mv, int Nv, int Kv, int layout, uint32_t* amax, const uint16_t* xo = nullptr, int ldo = 0, int n_out = 0) {
        return mixq_gemm_i8_pair_bf16(qx, q, p, p, xo, ldo, xo, ldo, n_out, nullptr, nullptr, y, ldy, Mv, Nv, Kv, layout, amax, nullptr, nullptr);
    };
    auto i4 = [&](const uint8_t* qx, uint16_t* y, int ldy, int Mv, int Nv, int Kv, int layout) {
        return mixq_gemm_i4_pair_bf16(qx, q4, p, p, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, y, ldy, Mv, Nv, Kv, layout, nullptr);
    };
    CHECK(mixq_gemm_set_config(-1) == MIXQ_OK);
    CHECK(i8(nullptr, p, 64, M, N, K, wf16, nullptr) == MIXQ_EINVAL);
    CHECK(i8(q, nullptr, 64, M, N, K, wf16, nullptr) == MIXQ_EINVAL);
    CHECK(i4(nullptr, p, 64, M, N, K, f6) == MIXQ_EINVAL);
    CHECK(i8(q, p, 64, M, N, K, 64, nullptr) == MIXQ_EINVAL);                                      // an unknown layout bit
    CHECK(i8(q, p, 64, M, N, K, f6, nullptr) == MIXQ_EINVAL);                                      // FP6 codes are the 4-bit entry's
    CHECK(i8(q, p, 64, M, N, K, MIXQ_X_PACKED | MIXQ_W_PACKED, pm) == MIXQ_EINVAL);                // row_amax beside a layout without the side output
    CHECK(i8(q, p, 64, M, N, K, MIXQ_X_PACKED | MIXQ_W_PACKED, nullptr) == MIXQ_ESHAPE);
    CHECK(i8(q, p, 64, M, N, K, 0, nullptr) == MIXQ_ESHAPE);
    CHECK(i4(q4, p, 64, M, N, K, wf16) == MIXQ_ESHAPE);
    CHECK(i4(q4, p, 64, M, N, K, MIXQ_X_PACKED | MIXQ_W_PACKED) == MIXQ_ESHAPE);
    CHECK(i8(q, p, 64, M, N, 96, wf16, nullptr) == MIXQ_ESHAPE);                                   // K % 64
    CHECK(i4(q4, p, 64, M, N, 192, f6) == MIXQ_ESHAPE);                                            // 4-bit: K % 128
    CHECK(i8(q, p, 64, M, 136, K, wf16, nullptr) == MIXQ_ESHAPE);                                  // N % 16
    CHECK(i8(q, p, 60, M, N, K, wf16, nullptr) == MIXQ_ESHAPE);                                    // ldy < N / 2
    CHECK(i8(q, p, 64, M, N, K, wf16, nullptr, p, 8, 3) == MIXQ_ESHAPE);                           // outlier stride below the padded width
    CHECK(i8(q, p8 - 2, 64, M, N, K, wf16, nullptr) == MIXQ_EINVAL);                               // y 4-byte aligned only
    CHECK(i8(q, p, 64, M, N, K, wf16, nullptr, p8, 16, 3) == MIXQ_EINVAL);                         // x_out / w_out 8-byte aligned only
    CHECK(i8(q, p, 64, 0, N, K, wf16, pm) == MIXQ_OK);                                             // M == 0: every check, no launch
    CHECK(i8(nullptr, nullptr, 64, 0, N, K, wf16, nullptr) == MIXQ_OK);
    CHECK(i4(q4, p, 64, 0, N, K, f6) == MIXQ_OK);
    CHECK(i8(q, p, 64, 0, N, 96, wf16, nullptr) == MIXQ_ESHAPE);                                   // ... the shape checks included
    CHECK(mixq_gemm_pair_supported_bf16(M, N, K, 8, wf16) == 1);
    CHECK(mixq_gemm_pair_supported_bf16(M, N, K, 4, f6) == 1);
    CHECK(mixq_gemm_pair_supported_bf16(M, N, 96, 8, wf16) == 0);
    CHECK(mixq_gemm_pair_supported_bf16(M, N, K, 8, MIXQ_X_PACKED | MIXQ_W_PACKED) == 0);
    CHECK(mixq_gemm_pair_supported_bf16(M, N, K, 4, wf16) == 0);
    CHECK(mixq_gemm_pair_supported_bf16(M, 136, K, 8, wf16) == 0);
    CHECK(mixq_gemm_pair_supported_bf16(0, N, K, 8, wf16) == 0);
    CHECK(mixq_gemm_pair_supported_bf16(M, N, K, 5, wf16) == 0);
    // forced configurations: every id either has the paired bf16 form (the empty problem is then MIXQ_OK) or is refused ahead of M == 0
    int with8 = 0, with6 = 0;
    for (int c = 0; c < mixq_gemm_num_configs(); ++c) {
        CHECK(mixq_gemm_set_config(c) == MIXQ_OK);
        const int r8 = i8(q, p, 64, 0, N, K, wf16, nullptr), r6 = i4(q4, p, 64, 0, N, K, f6);
        CHECK(r8 == MIXQ_OK || r8 == MIXQ_EINVAL);
        CHECK(r6 == MIXQ_OK || r6 == MIXQ_EINVAL);
        with8 += r8 == MIXQ_OK; with6 += r6 == MIXQ_OK;
    }
    CHECK(mixq_gemm_set_config(-1) == MIXQ_OK);
    CHECK(with8 == 5 && with6 == 4);
}

int main() {
    CHECK(mixq_version() > 0);
    norm_bf16_host_paths();
    pair_bf16_host_paths();
    int ngpu = 0;
    if (hipGetDeviceCount(&ngpu) != hipSuccess || ngpu == 0) {                  // (the rest needs device memory)
        (void)hipGetLastError();
        printf(g_fail ? "asan_capi: no GPU, host-only part: %d check(s) FAILED\n" : "asan_capi: no GPU, host-only part: all checks passed\n", g_fail);
        return g_fail ? 1 : 0;
    }
    char info[64];
    CHECK(mixq_version() > 0);
    CHECK(mixq_device_info(info, 8) == MIXQ_OK && strlen(info) < 8);          // (truncated, terminated)
    CHECK(mixq_device_info(info, sizeof(info)) == MIXQ_OK);
    CHECK(mixq_device_info(nullptr, 16) != MIXQ_OK);
    printf("device: %s\n", info);

    const int M = 100, K = 512, N = 264, n = 5, cap = 16;
    std::vector<uint16_t> hx(static_cast<size_t>(M) * K);
    for (auto& v : hx) v = f2h((static_cast<int>(rnd() % 2001) - 1000) / 250.f);
    std::vector<int32_t> hind = {7, 300, 64, 511, 33};                         // unsorted, as `ind` is after an append
    hind.resize(cap, K - 1);
    for (int r = 0; r < M; ++r) for (int j = 0; j < n; ++j) hx[static_cast<size_t>(r) * K + hind[j]] = f2h(40.f + r);
    Dev<uint16_t> x(hx.size()), x2(hx.size()), xs(M), xs2(M), xo(static_cast<size_t>(M) * cap), xo2(static_cast<size_t>(M) * cap), out(hx.size());
    Dev<int32_t> ind(cap), ndev(1), flag(1), cnt(1), indout(K);
    Dev<uint8_t> q(static_cast<size_t>(112) * K), q2(static_cast<size_t>(112) * K), colflags(K);
    ind.up(hind); ndev.up({n});
    const std::vector<uint32_t> hmap = kept_map(hind, n, K);
    Dev<uint32_t> map(hmap.size()); map.up(hmap);
    const int map_words = static_cast<int>(hmap.size());
    CHECK(map_words == mixq_kept_map_words(K));

    // ---- quantise passes: plain / packed, empty, rejected -------------------------------------------------------------------------------
    x.up(hx);
    CHECK(mixq_find_row_scale(x.p, xs.p, q.p, M, K, K, 8, MIXQ_FMT_PLAIN, nullptr) == MIXQ_OK);
    CHECK(mixq_find_row_scale(x.p, xs.p, q.p, M, K, K, 8, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
    CHECK(mixq_find_row_scale(x.p, xs.p, q.p, M, K, K, 4, MIXQ_FMT_PLAIN, nullptr) == MIXQ_OK);
    CHECK(mixq_find_row_scale(x.p, xs.p, q.p, 0, K, K, 8, MIXQ_FMT_PLAIN, nullptr) == MIXQ_OK);
    CHECK(mixq_find_row_scale(nullptr, nullptr, nullptr, 0, K, K, 8, MIXQ_FMT_PLAIN, nullptr) == MIXQ_OK);   // empty inputs may carry null pointers
    CHECK(mixq_find_row_scale(nullptr, xs.p, q.p, M, K, K, 8, MIXQ_FMT_PLAIN, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_find_row_scale(x.p, xs.p, q.p, M, K, K, 5, MIXQ_FMT_PLAIN, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_find_row_scale(x.p, xs.p, q.p, M, 100, 104, 8, MIXQ_FMT_PLAIN, nullptr) == MIXQ_ESHAPE);
    CHECK(mixq_find_row_scale(x.p, xs.p, q.p, M, K, K, 8, 9, nullptr) == MIXQ_EINVAL);
    HIPOK(hipDeviceSynchronize());
    // the in-kernel mask route against the kept-map route, device count below the capacity of `ind`
    x.up(hx); x2.up(hx);
    CHECK(mixq_quant_fused(x.p, ind.p, cap, ndev.p, xs.p, q.p, xo.p, flag.p, M, K, K, cap, 8, 6.f, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
    CHECK(mixq_quant_fused_masked(x2.p, ind.p, cap, ndev.p, map.p, map_words, xs2.p, q2.p, xo2.p, flag.p, M, K, K, cap, 8, 6.f, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
    HIPOK(hipDeviceSynchronize());
    CHECK(x.down() == x2.down() && xs.down() == xs2.down() && xo.down() == xo2.down());
    {   // (the packed images are block-major and their pad rows are never written: compare the M rows of the plain matrices)
        Dev<uint8_t> pa(static_cast<size_t>(M) * K), pb(static_cast<size_t>(M) * K);
        CHECK(mixq_unpack_operand(q.p, pa.p, M, K, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
        CHECK(mixq_unpack_operand(q2.p, pb.p, M, K, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
        HIPOK(hipDeviceSynchronize());
        CHECK(pa.down() == pb.down());
    }
    CHECK(mixq_quant_fused_masked(x2.p, ind.p, cap, ndev.p, map.p, (K + 31) / 32 + 1, xs2.p, q2.p, xo2.p, flag.p, M, K, K, cap, 8, 6.f, MIXQ_FMT_P16X64, nullptr) == MIXQ_EINVAL);   // (round 4's layout: bits + count only)
    CHECK(mixq_quant_fused_masked(x2.p, ind.p, cap, ndev.p, nullptr, 0, xs2.p, q2.p, xo2.p, flag.p, M, K, K, cap, 8, 6.f, MIXQ_FMT_P16X64, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_quant_fused(x.p, ind.p, n, nullptr, xs.p, q.p, nullptr, flag.p, M, K, K, cap, 8, 6.f, MIXQ_FMT_PLAIN, nullptr) == MIXQ_EINVAL);   // n > 0 needs x_out
    CHECK(mixq_quant_fused(x.p, ind.p, n, nullptr, xs.p, q.p, xo.p, flag.p, M, K, K, 3, 8, 6.f, MIXQ_FMT_PLAIN, nullptr) == MIXQ_EINVAL);        // ldo < n
    CHECK(mixq_quant_fused(x.p, nullptr, 0, nullptr, xs.p, q.p, nullptr, nullptr, M, K, K, 0, 4, 6.f, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
    x.up(hx);
    CHECK(mixq_extract_outliers_zero(x.p, ind.p, n, xo.p, M, K, K, cap, nullptr) == MIXQ_OK);
    CHECK(mixq_extract_outliers_zero(x.p, ind.p, n, xo.p, M, K, K, 2, nullptr) == MIXQ_EINVAL);
    x.up(hx);
    CHECK(mixq_detect_outlier_cols(x.p, 6.f, colflags.p, indout.p, cnt.p, M, K, K, nullptr) == MIXQ_OK);
    HIPOK(hipDeviceSynchronize());
    CHECK(cnt.down()[0] == n);
    CHECK(mixq_detect_outlier_cols(x.p, 6.f, nullptr, indout.p, cnt.p, M, K, K, nullptr) == MIXQ_EINVAL);

    // ---- weights: quantised matrix, re-tiling both ways, column dequantisation ---------------------------------------------------------
    std::vector<int8_t> hw(static_cast<size_t>(N) * K);
    for (auto& v : hw) v = static_cast<int8_t>(static_cast<int>(rnd() % 255) - 127);
    std::vector<uint16_t> hsw(N), hbias(N);
    for (int i = 0; i < N; ++i) { hsw[i] = f2h(0.001f + (rnd() % 100) * 1e-5f); hbias[i] = f2h((static_cast<int>(rnd() % 200) - 100) / 100.f); }
    const int N16 = (N + 15) / 16 * 16;
    Dev<int8_t> w(hw.size()), wback(hw.size());
    Dev<uint8_t> wp(static_cast<size_t>(N16) * K), wf(static_cast<size_t>(N16) * K);
    Dev<uint16_t> sw(N), bias(N), wo(static_cast<size_t>(N) * cap), y(static_cast<size_t>(M) * N), y2(static_cast<size_t>(M) * N), y3(static_cast<size_t>(M) * N);
    w.up(hw); sw.up(hsw); bias.up(hbias);
    CHECK(mixq_pack_operand(w.p, wp.p, N, K, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
    CHECK(mixq_pack_operand(w.p, wf.p, N, K, MIXQ_FMT_F16X64, nullptr) == MIXQ_OK);
    CHECK(mixq_unpack_operand(wf.p, wback.p, N, K, MIXQ_FMT_F16X64, nullptr) == MIXQ_OK);
    HIPOK(hipDeviceSynchronize());
    CHECK(wback.down() == hw);
    CHECK(mixq_pack_operand(w.p, wp.p, N, 100, MIXQ_FMT_P16X64, nullptr) == MIXQ_ESHAPE);
    CHECK(mixq_pack_operand(w.p, wp.p, N, K, 7, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_pack_operand(nullptr, wp.p, N, K, MIXQ_FMT_P16X64, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_pack_p16x64(w.p, wp.p, N, K, nullptr) == MIXQ_OK);
    CHECK(mixq_dequant_weight_cols(w.p, sw.p, ind.p, n, wo.p, N, K, cap, 8, nullptr) == MIXQ_OK);
    CHECK(mixq_dequant_weight_cols(w.p, sw.p, ind.p, n, wo.p, N, K, 2, 8, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_dequant_weight_cols(w.p, sw.p, ind.p, 0, wo.p, N, K, cap, 8, nullptr) == MIXQ_OK);

    // ---- fused GEMM: plain operands, P16X64 pair, fragment-order weights - one result ----------------------------------------------------
    x.up(hx);
    Dev<uint8_t> qplain(static_cast<size_t>(M) * K);
    CHECK(mixq_quant_fused(x.p, ind.p, cap, ndev.p, xs.p, qplain.p, xo.p, flag.p, M, K, K, cap, 8, 6.f, MIXQ_FMT_PLAIN, nullptr) == MIXQ_OK);
    x.up(hx);
    CHECK(mixq_quant_fused(x.p, ind.p, cap, ndev.p, xs.p, q.p, xo.p, flag.p, M, K, K, cap, 8, 6.f, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_i8_fused(reinterpret_cast<int8_t*>(qplain.p), w.p, xs.p, sw.p, xo.p, cap, wo.p, cap, cap, ndev.p, nullptr, 0, bias.p, y.p, N, M, N, K, MIXQ_ACT_NONE, 0, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_i8_fused(reinterpret_cast<int8_t*>(q.p), reinterpret_cast<int8_t*>(wp.p), xs.p, sw.p, xo.p, cap, wo.p, cap, cap, ndev.p, nullptr, 0, bias.p, y2.p, N, M, N, K, MIXQ_ACT_NONE, MIXQ_X_PACKED | MIXQ_W_PACKED, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_i8_fused(reinterpret_cast<int8_t*>(q.p), reinterpret_cast<int8_t*>(wf.p), xs.p, sw.p, xo.p, cap, wo.p, cap, cap, ndev.p, nullptr, 0, bias.p, y3.p, N, M, N, K, MIXQ_ACT_NONE, MIXQ_X_PACKED | MIXQ_W_F16X64, nullptr) == MIXQ_OK);
    HIPOK(hipDeviceSynchronize());
    { auto a = y.down(); CHECK(a == y2.down() && a == y3.down()); float s = 0; for (auto v : a) s += h2f(v); CHECK(s == s); }
    CHECK(mixq_gemm_i8_fused(reinterpret_cast<int8_t*>(q.p), reinterpret_cast<int8_t*>(wf.p), xs.p, sw.p, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, y3.p, N, M, N, 100, MIXQ_ACT_NONE, MIXQ_X_PACKED | MIXQ_W_F16X64, nullptr) == MIXQ_ESHAPE);
    CHECK(mixq_gemm_i8_fused(nullptr, reinterpret_cast<int8_t*>(wf.p), xs.p, sw.p, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, y3.p, N, M, N, K, MIXQ_ACT_NONE, MIXQ_X_PACKED | MIXQ_W_F16X64, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_gemm_i8_fused(reinterpret_cast<int8_t*>(q.p), reinterpret_cast<int8_t*>(wf.p), xs.p, sw.p, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, y3.p, N, 0, N, K, MIXQ_ACT_NONE, MIXQ_X_PACKED | MIXQ_W_F16X64, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_i8_fused(reinterpret_cast<int8_t*>(q.p), reinterpret_cast<int8_t*>(wf.p), xs.p, sw.p, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, y3.p, N, M, N, K, MIXQ_ACT_SILU_MUL, MIXQ_X_PACKED | MIXQ_W_F16X64, nullptr) != MIXQ_OK);   // (the multiplier is required)
    (void)mixq_gemm_amax_supported(M, N, K, MIXQ_X_PACKED | MIXQ_W_F16X64);

    // ---- the whole forward on a KEPT argument block: re-used, then edited (another batch size, the kept-map route) -----------------------
    mixq_linear_args a;
    memset(&a, 0, sizeof(a));
    a.x = x.p; a.ldx = K; a.ind = ind.p; a.n_cap = cap; a.n_dev = ndev.p; a.x_scale = xs.p; a.q_x = q.p; a.x_out = xo.p; a.ldxo = cap; a.flag = flag.p;
    a.q_w = wf.p; a.scale_col = sw.p; a.w_out = wo.p; a.ldwo = cap; a.bias = bias.p; a.y = y2.p; a.ldy = N;
    a.M = M; a.N = N; a.K = K; a.bit = 8; a.sigma = 6.f; a.act = MIXQ_ACT_NONE; a.qfmt = MIXQ_FMT_P16X64; a.wfmt = MIXQ_FMT_F16X64;
    for (int rep = 0; rep < 3; ++rep) {
        x.up(hx);
        CHECK(mixq_linear_forward(&a, nullptr) == MIXQ_OK);
        HIPOK(hipDeviceSynchronize());
        CHECK(y2.down() == y.down());
    }
    a.col_mask = map.p; a.col_mask_words = map_words;                          // the frozen layer's kept outlier map
    x.up(hx);
    CHECK(mixq_linear_forward(&a, nullptr) == MIXQ_OK);
    HIPOK(hipDeviceSynchronize());
    CHECK(y2.down() == y.down());
    a.M = 17;                                                                  // a decode-sized batch on the same block
    x.up(hx);
    CHECK(mixq_linear_forward(&a, nullptr) == MIXQ_OK);
    HIPOK(hipDeviceSynchronize());
    { auto full = y.down(), part = y2.down(); CHECK(memcmp(full.data(), part.data(), static_cast<size_t>(17) * N * 2) == 0); }
    a.M = 0;
    CHECK(mixq_linear_forward(&a, nullptr) == MIXQ_OK);
    a.M = M; a.bit = 3;
    CHECK(mixq_linear_forward(&a, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_linear_forward(nullptr, nullptr) == MIXQ_EINVAL);
    a.bit = 8; a.qfmt = MIXQ_FMT_PLAIN;                                        // fragment-order weights need P16X64 activations
    CHECK(mixq_linear_forward(&a, nullptr) != MIXQ_OK);

    // ---- RMSNorm in front of the path -----------------------------------------------------------------------------------------------------
    std::vector<uint16_t> hg(K);
    for (auto& v : hg) v = f2h(0.5f + (rnd() % 100) / 100.f);
    Dev<uint16_t> g(K); g.up(hg);
    x.up(hx);
    CHECK(mixq_rmsnorm(x.p, g.p, out.p, M, K, K, K, 1e-5f, nullptr) == MIXQ_OK);
    CHECK(mixq_rmsnorm(x.p, g.p, out.p, M, K, K, K - 8, 1e-5f, nullptr) == MIXQ_ESHAPE);
    CHECK(mixq_rmsnorm_quant_fused(x.p, g.p, out.p, ind.p, cap, ndev.p, xs.p, q.p, xo.p, flag.p, M, K, K, K, cap, 1e-5f, 8, 6.f, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
    CHECK(mixq_rmsnorm_quant_fused_masked(x.p, g.p, x2.p, ind.p, cap, ndev.p, map.p, map_words, xs2.p, q2.p, xo2.p, flag.p, M, K, K, K, cap, 1e-5f, 8, 6.f, MIXQ_FMT_P16X64, nullptr) == MIXQ_OK);
    HIPOK(hipDeviceSynchronize());
    CHECK(out.down() == x2.down() && xs.down() == xs2.down() && xo.down() == xo2.down());
    CHECK(mixq_rmsnorm_quant_fused(x.p, g.p, out.p, ind.p, n, nullptr, xs.p, q.p, nullptr, flag.p, M, K, K, K, cap, 1e-5f, 8, 6.f, MIXQ_FMT_PLAIN, nullptr) == MIXQ_EINVAL);

    // ---- weight-only W8A16 -------------------------------------------------------------------------------------------------------------------
    std::vector<int8_t> hkn(static_cast<size_t>(K) * N);
    for (auto& v : hkn) v = static_cast<int8_t>(static_cast<int>(rnd() % 255) - 127);
    Dev<int8_t> kn(hkn.size()); kn.up(hkn);
    Dev<uint8_t> w16(static_cast<size_t>(N16) * K);
    x.up(hx);
    CHECK(mixq_pack_w8a16(kn.p, w16.p, K, N, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_w8a16(x.p, K, w16.p, sw.p, bias.p, y3.p, N, M, N, K, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_w8a16(x.p, K, w16.p, sw.p, bias.p, y3.p, N, 1, N, K, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_w8a16(x.p, K, w16.p, sw.p, bias.p, y3.p, N, M, N, 100, nullptr) == MIXQ_ESHAPE);
    HIPOK(hipDeviceSynchronize());
    // ... with an addend (ABI 1.3): NULL is the call above, a zero addend with a pad (lda = N + 8) leaves its bytes; stride, pointer, M == 0
    CHECK(mixq_gemm_w8a16(x.p, K, w16.p, sw.p, bias.p, y3.p, N, M, N, K, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, nullptr, 0, bias.p, y2.p, N, M, N, K, nullptr) == MIXQ_OK);
    HIPOK(hipDeviceSynchronize());
    CHECK(y2.down() == y3.down());
    Dev<uint16_t> add(static_cast<size_t>(M) * (N + 8));                       // (zero-filled)
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, add.p, N + 8, bias.p, y2.p, N, M, N, K, nullptr) == MIXQ_OK);
    HIPOK(hipDeviceSynchronize());
    CHECK(y2.down() == y3.down());
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, add.p, N + 8, bias.p, y2.p, N, 1, N, K, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, add.p, N + 8, bias.p, y2.p, N, 0, N, K, nullptr) == MIXQ_OK);
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, add.p, N - 4, bias.p, y2.p, N, M, N, K, nullptr) == MIXQ_ESHAPE);       // lda < N
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, add.p, N + 2, bias.p, y2.p, N, M, N, K, nullptr) == MIXQ_ESHAPE);       // lda % 4
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, add.p, N - 4, bias.p, y2.p, N, 0, N, K, nullptr) == MIXQ_ESHAPE);       // ... checked at M == 0 too
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, add.p + 2, N + 8, bias.p, y2.p, N, M, N, K, nullptr) == MIXQ_EINVAL);   // base 4-byte aligned
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, add.p + 2, N + 8, bias.p, y2.p, N, 0, N, K, nullptr) == MIXQ_EINVAL);
    CHECK(mixq_gemm_w8a16_addend(x.p, K, w16.p, sw.p, add.p + 2, N - 4, bias.p, y2.p, N, M, N, 100, nullptr) == MIXQ_ESHAPE);  // K % 64 with a bad addend: as without
    CHECK(mixq_gemm_w8a16_addend(nullptr, K, w16.p, sw.p, add.p, N + 8, bias.p, y2.p, N, M, N, K, nullptr) == MIXQ_EINVAL);
    HIPOK(hipDeviceSynchronize());

    printf(g_fail ? "asan_capi: %d check(s) FAILED\n" : "asan_capi: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
