// qc_lds_probe.hip -- the LDS update of k_fq_cycle_hist (pyfastx_amd/csrc/fx_fastq_qc.hpp) on its own, no global loads (not
// part of the product).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o /tmp/qc_lds_probe tools/qc_lds_probe.hip && /tmp/qc_lds_probe
// Every lane owns a row of 51 words in a 13 KiB histogram per wave, as in the kernel (four waves per workgroup, three
// workgroups per CU), and adds 1 << (16 * (bin & 1)) to word bin >> 1 of its row, bins from a small per-lane generator over
// 4 or 36 values (the skewed and the uniform quality distributions).  Variant 0: ds_add_u32 without a return value; variant 1:
// ds_read_b32, add, ds_write_b32.  Prints ms and shader cycles per wave-instruction-sized update per CU, and checks the
// histogram's total against the number of updates.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

constexpr int ROW = 51, WAVES = 4;

template <int VARIANT>
__global__ __launch_bounds__(64 * WAVES) void k_probe(int iters, int values, unsigned long long *total) {
    __shared__ uint32_t hist[WAVES][64 * ROW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *row = hist[wv] + lane * ROW;
    for (int w = 0; w < ROW; ++w) row[w] = 0;
    uint32_t x = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 12345u;
    unsigned long long mine = 0;
    for (int it = 0; it < iters; it += 32) {
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            x = x * 1664525u + 1013904223u;
            const uint32_t bin = (x >> 24) % (uint32_t)values, inc = 1u << (16 * (bin & 1));
            if (VARIANT == 0) atomicAdd(&row[bin >> 1], inc);
            else row[bin >> 1] += inc;
        }
        if ((it & 0x7FE0) == 0x7FE0) {                       // before a 16-bit half can wrap
            for (int w = 0; w < ROW; ++w) { mine += (row[w] & 0xFFFFu) + (row[w] >> 16); row[w] = 0; }
        }
    }
    for (int w = 0; w < ROW; ++w) mine += (row[w] & 0xFFFFu) + (row[w] >> 16);
    atomicAdd(total, mine);
}

int main() {
    int n_cu = 256, clock_khz = 2400000;
    CK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, 0));
    CK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeClockRate, 0));
    unsigned long long *d_total, h_total;
    CK(hipMalloc(&d_total, 8));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int iters = 1 << 16, blocks = 3 * n_cu;
    for (int values : {4, 36})
        for (int variant = 0; variant < 2; ++variant) {
            float best = 1e30f;
            for (int rep = 0; rep < 4; ++rep) {                  // the first one warms up
                CK(hipMemset(d_total, 0, 8));
                CK(hipEventRecord(e0));
                if (variant == 0) hipLaunchKernelGGL(k_probe<0>, dim3(blocks), dim3(64 * WAVES), 0, 0, iters, values, d_total);
                else hipLaunchKernelGGL(k_probe<1>, dim3(blocks), dim3(64 * WAVES), 0, 0, iters, values, d_total);
                CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                if (rep && ms < best) best = ms;
            }
            CK(hipMemcpy(&h_total, d_total, 8, hipMemcpyDeviceToHost));
            const double updates = (double)blocks * WAVES * iters;            // wave-instruction-sized updates
            const bool ok = h_total == (unsigned long long)blocks * WAVES * 64ull * iters;
            printf("{\"tool\": \"qc_lds_probe\", \"values\": %d, \"variant\": \"%s\", \"ms\": %.3f, \"cycles_per_wave_update_per_cu\": %.1f, \"total_ok\": %s}\n",
                   values, variant == 0 ? "ds_add_u32" : "read_add_write", best, best * 1e-3 * clock_khz * 1e3 / (updates / n_cu), ok ? "true" : "false");
        }
    return 0;
}
