// What a thin gather costs the vector-memory address unit: a 64-lane buffer_load_dword from a 2 MB
// table (the decoder's global lookup) when
//   full   : every lane's offset is in range (random words of the table);
//   oob k  : k of the 64 lanes are in range, the rest past num_records (they return 0 without a memory
//            access -- how the decoder's lanes that resolved in LDS issue today);
//   exec k : the same k lanes active under EXEC, the rest masked off (EXEC set by hand around the loads).
// All three run the same instruction stream (one asm block of 8 independent loads and a wait; `full` and
// `oob` with EXEC all ones), 16 waves per CU on every CU, table L2-resident: instruction throughput, not
// latency. Every access is in bounds or returns 0 by the buffer rule, nothing is stored but one sink word.
// Reported per case: cycles per wave-instruction per CU from the waves' own cycle counters (s_memtime,
// mean over waves) and, beside it, from the event time at the clock the 100 MHz counter implies.
// build: hipcc --offload-arch=gfx950 -O3 mb_gather_thin.hip -o mbgt
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s\n", hipGetErrorString(e_)); return 1; } } while (0)

typedef int v4i __attribute__((ext_vector_type(4)));
constexpr uint32_t kTableBytes = 2u << 20;
constexpr int ILP = 8;

// mode 0 full, 1 oob, 2 exec; k lanes in range (modes 1, 2)
__global__ __launch_bounds__(1024) void gather(const uint32_t* tab, int mode, uint32_t k, int iters, uint64_t* cyc,
                                               uint64_t* ref, uint32_t* sink) {
    const uint32_t lane = threadIdx.x & 63;
    const uintptr_t p = reinterpret_cast<uintptr_t>(tab);
    v4i rsrc;
    rsrc.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)p);
    rsrc.y = __builtin_amdgcn_readfirstlane((int)(uint32_t)(p >> 32));  // stride 0: raw buffer
    rsrc.z = __builtin_amdgcn_readfirstlane((int)kTableBytes);          // num_records, bytes
    rsrc.w = __builtin_amdgcn_readfirstlane(0x00020000);
    const bool in = mode == 0 || (lane * k) % 64u < k;  // k lanes, spread over the wave
    const uint64_t all = ~0ull;
    const uint64_t em = mode == 2 ? __ballot(in) : all;
    const uint32_t emlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)em);
    const uint32_t emhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(em >> 32));
    const uint64_t emask = ((uint64_t)emhi << 32) | emlo;
    uint32_t acc = 0, seed = blockIdx.x * 7919u + threadIdx.x * 104729u;
    const uint64_t t0 = clock64(), r0 = wall_clock64();
    for (int i = 0; i < iters; ++i) {
        uint32_t off[ILP], v[ILP];
#pragma unroll
        for (int c = 0; c < ILP; ++c) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t o = (seed >> 4) & (kTableBytes - 4u);
            off[c] = in ? o : o + 2u * kTableBytes;  // past num_records: 0, no memory access
            v[c] = 0;
        }
        uint64_t save;
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_mov_b64 exec, %[m]\n\t"
            "buffer_load_dword %[v0], %[o0], %[r], 0 offen\n\t"
            "buffer_load_dword %[v1], %[o1], %[r], 0 offen\n\t"
            "buffer_load_dword %[v2], %[o2], %[r], 0 offen\n\t"
            "buffer_load_dword %[v3], %[o3], %[r], 0 offen\n\t"
            "buffer_load_dword %[v4], %[o4], %[r], 0 offen\n\t"
            "buffer_load_dword %[v5], %[o5], %[r], 0 offen\n\t"
            "buffer_load_dword %[v6], %[o6], %[r], 0 offen\n\t"
            "buffer_load_dword %[v7], %[o7], %[r], 0 offen\n\t"
            "s_mov_b64 exec, %[sv]\n\t"
            "s_waitcnt vmcnt(0)"
            : [sv] "=&s"(save), [v0] "+v"(v[0]), [v1] "+v"(v[1]), [v2] "+v"(v[2]), [v3] "+v"(v[3]), [v4] "+v"(v[4]),
              [v5] "+v"(v[5]), [v6] "+v"(v[6]), [v7] "+v"(v[7])
            : [m] "s"(emask), [r] "s"(rsrc), [o0] "v"(off[0]), [o1] "v"(off[1]), [o2] "v"(off[2]), [o3] "v"(off[3]),
              [o4] "v"(off[4]), [o5] "v"(off[5]), [o6] "v"(off[6]), [o7] "v"(off[7])
            : "memory");
#pragma unroll
        for (int c = 0; c < ILP; ++c) acc += v[c];
    }
    const uint64_t t1 = clock64(), r1 = wall_clock64();
    if (lane == 0) {
        const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        cyc[w] = t1 - t0;
        ref[w] = r1 - r0;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

int main() {
    std::vector<uint32_t> h(kTableBytes / 4);
    for (uint32_t i = 0; i < h.size(); ++i) h[i] = (i * 2654435761u) >> 7;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount, waves = 16;
    uint32_t *tab, *sink;
    uint64_t *cyc, *ref;
    CK(hipMalloc(&tab, kTableBytes));
    CK(hipMalloc(&sink, 64));
    CK(hipMalloc(&cyc, 8ull * cus * waves));
    CK(hipMalloc(&ref, 8ull * cus * waves));
    CK(hipMemcpy(tab, h.data(), kTableBytes, hipMemcpyHostToDevice));
    std::vector<uint64_t> hc((size_t)cus * waves), hr((size_t)cus * waves);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const int iters = 2048;
    const struct { int mode; uint32_t k; const char* name; } cases[] = {
        {0, 64, "full   "}, {1, 20, "oob  20"}, {2, 20, "exec 20"}, {1, 5, "oob   5"}, {2, 5, "exec  5"}};
    for (const auto& c : cases) {
        double best_ms = 1e9, best_cyc = 0, best_ref = 0;
        for (int rep = 0; rep < 4; ++rep) {  // the first rep warms the table into L2
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(gather, dim3(cus), dim3(64 * waves), 0, 0, tab, c.mode, c.k, iters, cyc, ref, sink);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            CK(hipMemcpy(hc.data(), cyc, 8 * hc.size(), hipMemcpyDeviceToHost));
            CK(hipMemcpy(hr.data(), ref, 8 * hr.size(), hipMemcpyDeviceToHost));
            double sc = 0, sr = 0;
            for (size_t i = 0; i < hc.size(); ++i) { sc += (double)hc[i]; sr += (double)hr[i]; }
            if (rep > 0 && ms < best_ms) { best_ms = ms; best_cyc = sc / hc.size(); best_ref = sr / hr.size(); }
        }
        const double per_cu = (double)waves * iters * ILP;  // wave-instructions a CU issues
        const double ghz = best_cyc / (best_ref * 10.0);     // cycle counter against the 100 MHz counter
        printf("%s: %.3f ms; %.2f cycles/wave-instruction/CU by the cycle counter (%.0f cycles a wave, %.2f GHz "
               "against the 100 MHz counter); %.2f by the event time at that clock\n",
               c.name, best_ms, best_cyc / per_cu, best_cyc, ghz, best_ms * 1e-3 * ghz * 1e9 / per_cu);
    }
    return 0;
}
