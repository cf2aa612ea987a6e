// Issue rate of the integer multiplies and shift-adds of the backward kernel's drain and addressing against v_fma_f32 on MI355X:
// 16 independent chains per lane, ITER turns, one .. three waves per SIMD (the backward kernel runs at three).
// hipcc -O3 --offload-arch=gfx950 -o tools/micro/int_mul tools/micro/int_mul.hip && tools/micro/int_mul
// Prints, per instruction and occupancy, the time, the wave-instructions per clock and SIMD it implies at the clock the
// device reports, and the time relative to v_fma_f32 at the same occupancy (1.0 = full rate, 4.0 = quarter rate).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
enum Op { FMA_F32, MUL_LO_U32, MUL_HI_U32, MAD_U64_U32, MUL_U32_U24, LSHL_ADD_U32, LSHL_ADD_U64, N_OPS };
static const char *kNames[N_OPS] = {"v_fma_f32", "v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_mul_u32_u24", "v_lshl_add_u32", "v_lshl_add_u64"};
constexpr int kChains = 16;
template <int OP>
__global__ __launch_bounds__(256) void k(uint32_t *out, uint32_t a, uint32_t b, int iters) {
    uint32_t acc[kChains];
    uint64_t acc64[kChains];
    float accf[kChains];
#pragma unroll
    for (int j = 0; j < kChains; ++j) { acc[j] = threadIdx.x * 2654435761u + j; acc64[j] = ((uint64_t) acc[j] << 20) + j; accf[j] = (float) threadIdx.x + j; }
    const uint32_t av = a | 1u, bv = b + threadIdx.x;
    const uint64_t bv64 = ((uint64_t) b << 32) | threadIdx.x;
    const float af = 0.999f, bf = 0.001f * (float) a;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < kChains; ++j) {
            if (OP == FMA_F32) asm volatile("v_fma_f32 %0, %1, %0, %2" : "+v"(accf[j]) : "v"(af), "v"(bf));
            if (OP == MUL_LO_U32) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(acc[j]) : "v"(av));
            if (OP == MUL_HI_U32) asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(acc[j]) : "v"(av));
            if (OP == MAD_U64_U32) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc64[j]) : "v"(av), "v"(bv) : "vcc");
            if (OP == MUL_U32_U24) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(acc[j]) : "v"(av));
            if (OP == LSHL_ADD_U32) asm volatile("v_lshl_add_u32 %0, %0, 3, %1" : "+v"(acc[j]) : "v"(bv));
            if (OP == LSHL_ADD_U64) asm volatile("v_lshl_add_u64 %0, %0, 3, %1" : "+v"(acc64[j]) : "v"(bv64));
        }
    }
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < kChains; ++j) s += acc[j] + (uint32_t) acc64[j] + (uint32_t) (acc64[j] >> 32) + __float_as_uint(accf[j]);
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
typedef void (*Kern)(uint32_t *, uint32_t, uint32_t, int);
int main() {
    static const Kern kerns[N_OPS] = {k<FMA_F32>, k<MUL_LO_U32>, k<MUL_HI_U32>, k<MAD_U64_U32>, k<MUL_U32_U24>, k<LSHL_ADD_U32>, k<LSHL_ADD_U64>};
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 1; }
    const int simds = prop.multiProcessorCount * 4;
    const double clock_khz = prop.clockRate;
    constexpr int kMaxWaves = 3;
    uint32_t *out;
    if (hipMalloc(&out, sizeof(uint32_t) * 256 * (size_t) prop.multiProcessorCount * kMaxWaves) != hipSuccess) return 1;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int iters = 4096;
    printf("%s: %d CUs, %.0f MHz; %d chains per lane, %d turns\n", prop.name, prop.multiProcessorCount, clock_khz * 1e-3, kChains, iters);
    for (int waves = 1; waves <= kMaxWaves; ++waves) {
        const int blocks = prop.multiProcessorCount * waves;      // workgroups of four waves: `waves` per SIMD
        float fma_ms = 0.f;
        for (int op = 0; op < N_OPS; ++op) {
            float best = 1e30f;
            for (int rep = 0; rep < 3; ++rep) {
                hipEventRecord(e0);
                hipLaunchKernelGGL(kerns[op], dim3(blocks), dim3(256), 0, 0, out, 12345u, 678u, iters);
                hipEventRecord(e1);
                if (hipEventSynchronize(e1) != hipSuccess) { printf("launch failed\n"); return 1; }
                float ms; hipEventElapsedTime(&ms, e0, e1);
                if (rep > 0 && ms < best) best = ms;
            }
            if (op == FMA_F32) fma_ms = best;
            const double wave_insts = (double) blocks * 4 * iters * kChains;
            printf("%d waves per SIMD  %-15s %8.3f ms  %.3f wave-instructions per clock and SIMD  x%.2f of v_fma_f32\n", waves, kNames[op], best,
                   wave_insts / simds / (best * 1e-3 * clock_khz * 1e3), best / fma_ms);
        }
    }
    hipFree(out);
    return 0;
}
