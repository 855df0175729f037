// Which SIMD does wave i of a 256-thread block land on?  k_expand_dw gives its four waves unequal work by wave index (tile ownership in
// phase 1, output rows in phase 2); whether that makes one SIMD of every CU the bottleneck depends on the dispatcher's placement, which
// this program reads back: blocks of 256 threads with 35 KB of LDS (four per CU, the occupancy of the 6 x 32 fused layers), every wave
// reads the hardware-id registers and lane 0 stores them, with the block's dispatch index, through ordinary vector stores.
// Printed: the histogram (wave index in block -> SIMD id), alone and beside a second stream that runs an f32-MFMA GEMM; and, for
// candidate "rot" functions of the XCD-local block index q = blockIdx.x >> 3, how evenly the blocks that one CU received spread
// over the four values (share of a CU's blocks on its most frequent value: 0.25 is perfect, 1.0 is none).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o tools/ubench/bin/wave_placement tools/ubench/wave_placement.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define HW_ID_ALL (4 | (31 << 11))        // s_getreg simm16: register 4 (HW_ID), offset 0, 32 bits
#define XCC_ID_ALL (20 | (31 << 11))      // register 20 (XCC_ID)

__global__ __launch_bounds__(256) void k_place(unsigned* tab, int spin) {
    __shared__ float lds[35 * 256];                       // 35 KB: four blocks per CU
    const int tid = threadIdx.x, wave = tid >> 6;
    const unsigned hw = __builtin_amdgcn_s_getreg(HW_ID_ALL), xcc = __builtin_amdgcn_s_getreg(XCC_ID_ALL);
    // stay resident for a while (a few microseconds of dependent fp work through LDS) so that the CU fills to its four blocks
    float v = (float)tid;
    for (int i = 0; i < spin; i++) {
        lds[(tid + 256 * (i % 35)) % (35 * 256)] = v;
        __syncthreads();
        v = fmaf(v, 1.0001f, lds[(tid * 7 + i) % (35 * 256)]);
    }
    if ((tid & 63) == 0) {
        unsigned* t = tab + ((size_t)blockIdx.x * 4 + wave) * 2;
        t[0] = hw;
        t[1] = (xcc & 15u) | (v == 12345.678f ? 16u : 0u);      // (keeps the loop alive)
    }
}

// the co-runner: C = A B on the f32 MFMA, one 16 x 16 output tile per wave, operands straight from global memory
__global__ __launch_bounds__(256) void k_gemm(const float* A, const float* Bm, float* C, int M, int N, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
    const int tn = N / 16, tile = blockIdx.x * 4 + wave;
    if (tile >= (M / 16) * tn) return;
    const int m0 = tile / tn * 16, n0 = tile % tn * 16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k += 4)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[(size_t)(m0 + li) * K + k + kq], Bm[(size_t)(k + kq) * N + n0 + li], acc, 0, 0, 0);
    for (int r = 0; r < 4; r++) C[(size_t)(m0 + 4 * kq + r) * N + n0 + li] = acc[r];
}

static unsigned fold2(unsigned q) { unsigned r = 0; for (; q; q >>= 2) r ^= q; return r & 3; }
struct Cand { const char* name; unsigned (*f)(unsigned); };
static const Cand kCands[] = {
    {"0 (no rotation)", [](unsigned) { return 0u; }},
    {"q & 3", [](unsigned q) { return q & 3; }},
    {"(q >> 5) & 3", [](unsigned q) { return (q >> 5) & 3; }},
    {"(q + (q >> 5)) & 3", [](unsigned q) { return (q + (q >> 5)) & 3; }},
    {"xor of q's base-4 digits", fold2},
};

static void run(const char* title, int nblk, int spin, bool corun) {
    unsigned* tab; (void)hipMalloc(&tab, (size_t)nblk * 8 * 4); (void)hipMemset(tab, 0xff, (size_t)nblk * 8 * 4);
    hipStream_t s0, s1; (void)hipStreamCreate(&s0); (void)hipStreamCreate(&s1);
    const int M = 2048, N = 2048, K = 1024;
    float *A = nullptr, *Bm = nullptr, *C = nullptr;
    if (corun) {
        (void)hipMalloc(&A, (size_t)M * K * 4); (void)hipMalloc(&Bm, (size_t)K * N * 4); (void)hipMalloc(&C, (size_t)M * N * 4);
        (void)hipMemset(A, 0, (size_t)M * K * 4); (void)hipMemset(Bm, 0, (size_t)K * N * 4);
        for (int i = 0; i < 4; i++) hipLaunchKernelGGL(k_gemm, dim3(M / 16 * (N / 16) / 4), dim3(256), 0, s1, A, Bm, C, M, N, K);
    }
    hipLaunchKernelGGL(k_place, dim3(nblk), dim3(256), 0, s0, tab, spin);
    if (hipDeviceSynchronize() != hipSuccess) { printf("HIP error\n"); exit(3); }
    std::vector<unsigned> h((size_t)nblk * 8);
    (void)hipMemcpy(h.data(), tab, h.size() * 4, hipMemcpyDeviceToHost);
    long hist[4][4] = {};
    long same_block_distinct = 0;                         // blocks whose four waves sit on four different SIMDs
    std::map<unsigned, std::vector<unsigned>> per_cu;     // (xcc, se, sh, cu) -> XCD-local indices of its blocks
    std::map<unsigned, std::vector<unsigned>> w0_simd;    // ... -> the SIMD of wave 0 of each of its blocks
    for (int b = 0; b < nblk; b++) {
        unsigned seen = 0;
        for (int w = 0; w < 4; w++) {
            const unsigned hw = h[((size_t)b * 4 + w) * 2];
            hist[w][(hw >> 4) & 3]++; seen |= 1u << ((hw >> 4) & 3);
        }
        same_block_distinct += seen == 15u;
        const unsigned hw = h[(size_t)b * 8], xcc = h[(size_t)b * 8 + 1] & 15u;
        const unsigned cu = (xcc << 16) | (((hw >> 13) & 7) << 8) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15);
        per_cu[cu].push_back((unsigned)b >> 3);
        w0_simd[cu].push_back((hw >> 4) & 3);
    }
    printf("== %s: %d blocks of 4 waves, %zu CUs seen\n", title, nblk, per_cu.size());
    printf("   wave -> SIMD id   simd0   simd1   simd2   simd3\n");
    for (int w = 0; w < 4; w++) printf("   wave %d         %7ld %7ld %7ld %7ld\n", w, hist[w][0], hist[w][1], hist[w][2], hist[w][3]);
    printf("   blocks with their four waves on four different SIMDs: %ld of %d\n", same_block_distinct, nblk);
    {
        // the question itself, per CU: do the blocks that one CU received put their wave 0 on one SIMD?
        double worst = 0, mean = 0;
        for (auto& kv : w0_simd) {
            long cnt[4] = {};
            for (unsigned sd : kv.second) cnt[sd]++;
            const double share = (double)*std::max_element(cnt, cnt + 4) / (double)kv.second.size();
            worst = std::max(worst, share); mean += share;
        }
        printf("   per CU: share of its blocks whose wave 0 sits on the CU's most frequent SIMD for wave 0: mean %.3f, worst CU %.3f (0.25 = even, 1 = fixed)\n",
               mean / w0_simd.size(), worst);
    }
    for (const Cand& c : kCands) {
        double worst = 0, mean = 0;
        for (auto& kv : per_cu) {
            long cnt[4] = {};
            for (unsigned q : kv.second) cnt[c.f(q)]++;
            const double share = (double)*std::max_element(cnt, cnt + 4) / (double)kv.second.size();
            worst = std::max(worst, share); mean += share;
        }
        printf("   rot = %-26s share of a CU's blocks on its most frequent value: mean %.3f, worst CU %.3f\n", c.name, mean / per_cu.size(), worst);
    }
    if (!corun && nblk <= 1024) {
        int shown = 0;
        for (auto& kv : per_cu) {
            if (shown++ >= 4) break;
            printf("   CU %06x got XCD-local block indices:", kv.first);
            for (unsigned q : kv.second) printf(" %u", q);
            printf("   (SIMD of their wave 0:");
            for (unsigned sd : w0_simd[kv.first]) printf(" %u", sd);
            printf(")\n");
        }
    }
    (void)hipFree(tab); (void)hipFree(A); (void)hipFree(Bm); (void)hipFree(C);
    (void)hipStreamDestroy(s0); (void)hipStreamDestroy(s1);
}

int main() {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) { printf("no HIP device\n"); return 3; }
    run("one resident generation (4 blocks per CU), alone", 1024, 200, false);
    run("a b10-sized grid (3840 blocks), alone", 3840, 200, false);
    run("a b10-sized grid, beside a GEMM on a second stream", 3840, 200, true);
    return 0;
}
