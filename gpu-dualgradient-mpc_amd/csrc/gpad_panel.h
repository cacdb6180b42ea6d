// gpad_panel.h -- the pieces of the T-wave f32 MFMA panel shared by gpad_panel.hip (gpad_panel_kernel:
// a batch of independent solves) and gpad_loop_panel.hip (gpad_loop_panel_kernel: a queue of
// closed-loop packs): the vector types, the per-tile slots of the Algorithm-1 test and the skinny
// GEMM.  Both kernels run exactly this panel_gemm per (row tile, column), so their MFMA chains
// cannot drift apart.  The fragment layout is described at the top of gpad_panel.hip.
#pragma once

#include <hip/hip_runtime.h>

namespace gpad {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct PanelSlot {  // per wave (row tile), per instance partials of the Algorithm-1 test
    float violz[16], violh[16], wmin[16];
    double gap[16];
    float magh[16];  // max(|G_L zhat| + |pD|): test (B)'s rounding scale
};
// (A) nominated by the recursive u is decided on the direct G_L z (gpad_internal.h ViolMargin):
// the verification reuses violz / magh of the slots for max(G_L z + pD) / max(|G_L z| + |pD|).

// acc = A[tile t] (T k-blocks, streamed from L2 one block ahead) x B (LDS, fragment order).
// The MFMA k-order is ascending (block 0..T-1, step 0..3), i.e. the reference's sequential chain.
// A is read with buffer loads: one 32-bit lane offset (t*1 KiB + lane*16 B) in a VGPR and the
// k-block offset as a compile-time scalar, so the unrolled blocks cost no address registers.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 as_float4(u32x4 v) {
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z),
                       __uint_as_float(v.w));
}

template <int T>
__device__ __forceinline__ f32x4 panel_gemm(__amdgpu_buffer_rsrc_t PA, const float* Bl, int voff,
                                            int lane) {
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    float4 a[2], b[2];
    a[0] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, 0, 0));
    b[0] = *reinterpret_cast<const float4*>(Bl + lane * 4);
#pragma unroll
    for (int kb = 0; kb < T; ++kb) {
        const int cur = kb & 1, nxt = cur ^ 1;
        if (kb + 1 < T) {
            a[nxt] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(PA, voff, (kb + 1) * T * 1024, 0));
            b[nxt] = *reinterpret_cast<const float4*>(Bl + ((kb + 1) * 64 + lane) * 4);
        }
        // the next block's loads issue BEFORE this block's MFMAs (else the scheduler sinks them
        // below and waits on them at once: a full L2 round trip per k-block)
        __builtin_amdgcn_sched_barrier(0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].x, b[cur].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].y, b[cur].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].z, b[cur].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur].w, b[cur].w, acc, 0, 0, 0);
        asm volatile("" ::: "memory");  // keep the prefetch one k-block deep
    }
    return acc;
}

}  // namespace gpad
