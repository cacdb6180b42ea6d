// gpad_loop_kernels.inc -- the text of the two asynchronous loop kernels, included twice by gpad_loop.h:
// GPAD_LOOP_FK 0: gpad_loop_kernel<KA, KB, MODE> and gpad_loop_fleet_kernel<KA, KB>; 1: gpad_loop_farkas_kernel
// and gpad_loop_fleet_farkas_kernel, the same loops with the infeasibility certificate (gpad_farkas.h) after
// every fourth test of a solve (loop_post_b, loop_farkas).  Two inclusions for gpad_stream_solve.inc's reason:
// with nothing bound a kernel must be the code it has as a kernel of its own (tools/isa_diff.py).  The
// FarkasArgs is read from the kernarg segment at the event (lfargs()).
template <int KA, int KB, int MODE = kLoopShared>
#if GPAD_LOOP_FK
__global__ __launch_bounds__(kResidentMaxThreads) void gpad_loop_farkas_kernel(LoopArgs la, FarkasArgs) {
    constexpr int FKA = KA;
#else
__global__ __launch_bounds__(kResidentMaxThreads) void gpad_loop_kernel(LoopArgs la) {
    constexpr int FKA = 0;
#endif
    const SolveArgs<float>& a = la.s;
    constexpr int K = KA > KB ? KA : KB;
    constexpr int PA = (KA + 63) / 64 * 64, PB = (KB + 63) / 64 * 64;
    __shared__ __attribute__((aligned(16))) float w_l[2][PA];   // w per slot (broadcast to -ML rows)
    __shared__ __attribute__((aligned(16))) float zh_l[2][PB];  // zhat per slot (to G/L rows)
    __shared__ __attribute__((aligned(16))) float z_l[PB];      // z_{-1} of a fresh solve (u seed)
    __shared__ float gp_l[2][PB];                               // per slot: g_P of the -ML rows
    __shared__ float pd_l[2][PA];                               //           p_D of the G/L rows
    __shared__ CheckSlot slots[2][kResidentMaxThreads / 64];
    __shared__ CheckSlot vslots[kResidentMaxThreads / 64];  // verification of a nominated test (A)
    __shared__ int claim_l[2];
    __shared__ LoopLds L;

    DuoCtx c;
    c.tid = threadIdx.x;
    c.count = a.batch;
    c.G = gridDim.x;
    c.v0 = 0;
    c.fresh = true;
    c.use_tol = a.tol > 0.0;
    c.n = a.n;
    c.m = a.m;
    c.N = a.N;
    c.Kc = a.check_every;
    c.kc0 = c.Kc;
    c.nA = (c.n + 63) >> 6;
    c.nwaves = blockDim.x >> 6;
    {   // the G/L waves first (the older wave of each SIMD), as gpad_duo_kernel
        const int nB = c.nwaves - c.nA;
        c.isA = (c.tid >> 6) >= nB;
        c.row = c.isA ? c.tid - 64 * nB : c.tid;
        c.b0 = 0;
    }
    c.live = c.isA ? c.row < c.n : c.row < c.m;

    float r[K];
    {
        const int len = c.isA ? c.m : c.n;
        const float* __restrict__ Mt = c.isA ? a.MGt : a.GLt;
        const int ld = c.isA ? a.ldn : a.ldm;
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = (c.live && k < len) ? Mt[(size_t)k * ld + c.row] : 0.0f;
    }
    for (int i = c.tid; i < 2 * PA; i += blockDim.x) (&w_l[0][0])[i] = 0.0f;
    for (int i = c.tid; i < 2 * PB; i += blockDim.x) (&zh_l[0][0])[i] = 0.0f;
    for (int i = c.tid; i < PB; i += blockDim.x) z_l[i] = 0.0f;
    for (int i = c.tid; i < kResidentMaxThreads; i += blockDim.x) L.gm[i] = 0.0f;
    // Static start: slot 0 of workgroup b takes pack b, slot 1 pack G + b; later packs are claimed
    // from the counter.  (The grid is at most `batch` workgroups, so every slot 0 has a pack.)
    c.claim_base = 2 * c.G;
    if (c.tid == 0) {  // first claims of the queue (positions 2G, ...)
        claim_l[0] = c.claim_base + atomicAdd(a.qctr, 1);
        claim_l[1] = c.claim_base + atomicAdd(a.qctr, 1);
    }
    __syncthreads();
    LoopSlotOf<FKA != 0> s0, s1;
    s0.nextp = __builtin_amdgcn_readfirstlane(claim_l[0]);
    s1.nextp = __builtin_amdgcn_readfirstlane(claim_l[1]);
    loop_refill<KB, K, MODE, FKA != 0>(a, c, s0, blockIdx.x, &L.x[0][0][0], w_l[0], gp_l[0], pd_l[0], z_l, L.gm, r);
    loop_refill<KB, K, MODE, FKA != 0>(a, c, s1, blockIdx.x + c.G, &L.x[1][0][0], w_l[1], gp_l[1], pd_l[1], z_l, L.gm, r);
    while (s0.pos < c.count || s1.pos < c.count) {
        if (s0.pos >= c.count) {
            loop_solo<KA, KB, K, MODE, FKA>(a, c, s1, w_l[1], zh_l[1], gp_l[1], pd_l[1], slots[1], vslots, &claim_l[1],
                                            z_l, &L.x[1][0][0], L.u, L.gm, r);
            break;
        }
        if (s1.pos >= c.count) {
            loop_solo<KA, KB, K, MODE, FKA>(a, c, s0, w_l[0], zh_l[0], gp_l[0], pd_l[0], slots[0], vslots, &claim_l[0],
                                            z_l, &L.x[0][0][0], L.u, L.gm, r);
            break;
        }
        loop_step<KA, KB, K, MODE, FKA>(a, c, s0, s1, w_l[0], zh_l[0], gp_l[0], w_l[1], zh_l[1], gp_l[1], pd_l[1],
                                        slots[1], vslots, &claim_l[1], z_l, &L.x[1][0][0], L.u, L.gm, r);
        loop_step<KA, KB, K, MODE, FKA>(a, c, s1, s0, w_l[1], zh_l[1], gp_l[1], w_l[0], zh_l[0], gp_l[0], pd_l[0],
                                        slots[0], vslots, &claim_l[0], z_l, &L.x[0][0][0], L.u, L.gm, r);
    }
    // the run's max |g| (the certification floor): this workgroup's slot, workgroup 0 zeroes the rest
    LoopKernArgs& A = largs();
    if (A.gmax) {
        const float wm = wave_reduce(L.gm[c.tid], OpAbsmaxNan{});
        __syncthreads();  // (every lane has read its L.gm word)
        if ((c.tid & 63) == 0) L.gm[c.tid >> 6] = wm;
        __syncthreads();
        if (c.tid == 0) {
            float mx = 0.0f;
            for (int w = 0; w < c.nwaves; ++w) mx = absmax_nan(mx, L.gm[w]);
            A.gmax[blockIdx.x] = (double)mx;
        }
        if (blockIdx.x == 0)
            for (int i = c.G + c.tid; i < kAbsmaxMaxBlocks; i += blockDim.x) A.gmax[i] = 0.0;
    }
}

// =========================================================================================
// gpad_loop_fleet_kernel: the same loop for a fleet of distinct plants (per-pack -ML, G/L).
// =========================================================================================
// Two packs cannot share one set of row registers, so a workgroup holds ONE live slot and runs
// loop_solo on it: the resident kernel's loop with the step boundary above.  When the slot takes a
// pack -- workgroup b starts with pack b, later packs come from the queue (positions G, ...) -- it
// loads that pack's rows from MGt + p strideA / GLt + p strideB (loop_rows) and keeps them for the
// pack's `steps` steps, where the lockstep loop re-reads every pack's matrices at every step.  The
// ping-pong's latency hiding is gone; the host runs two workgroups per CU where they fit instead.
template <int KA, int KB>
#if GPAD_LOOP_FK
__global__ __launch_bounds__(kResidentMaxThreads) void gpad_loop_fleet_farkas_kernel(LoopArgs la, FarkasArgs) {
    constexpr int FKA = KA;
#else
__global__ __launch_bounds__(kResidentMaxThreads) void gpad_loop_fleet_kernel(LoopArgs la) {
    constexpr int FKA = 0;
#endif
    const SolveArgs<float>& a = la.s;
    constexpr int K = KA > KB ? KA : KB;
    constexpr int PA = (KA + 63) / 64 * 64, PB = (KB + 63) / 64 * 64;
    __shared__ __attribute__((aligned(16))) float w_l[PA];   // w (broadcast to -ML rows)
    __shared__ __attribute__((aligned(16))) float zh_l[PB];  // zhat (to G/L rows)
    __shared__ __attribute__((aligned(16))) float z_l[PB];   // z_{-1} of a fresh solve (u seed)
    __shared__ float gp_l[PB];                               // g_P of the -ML rows
    __shared__ float pd_l[PA];                               // p_D of the G/L rows
    __shared__ CheckSlot slots[kResidentMaxThreads / 64];
    __shared__ CheckSlot vslots[kResidentMaxThreads / 64];
    __shared__ int claim_l;
    __shared__ LoopLds L;  // (x[0], u, gm)

    const DuoCtx c = loop_ctx(a, (int)gridDim.x);
    float r[K];
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = 0.0f;
    for (int i = c.tid; i < PA; i += blockDim.x) w_l[i] = 0.0f;
    for (int i = c.tid; i < PB; i += blockDim.x) zh_l[i] = z_l[i] = 0.0f;
    for (int i = c.tid; i < kResidentMaxThreads; i += blockDim.x) L.gm[i] = 0.0f;
    if (c.tid == 0) claim_l = c.claim_base + atomicAdd(a.qctr, 1);  // first claim of the queue
    __syncthreads();
    LoopSlotOf<FKA != 0> s;
    s.nextp = __builtin_amdgcn_readfirstlane(claim_l);
    loop_refill<KB, K, kLoopFleet, FKA != 0>(a, c, s, blockIdx.x, &L.x[0][0][0], w_l, gp_l, pd_l, z_l, L.gm, r);
    loop_solo<KA, KB, K, kLoopFleet, FKA>(a, c, s, w_l, zh_l, gp_l, pd_l, slots, vslots, &claim_l, z_l, &L.x[0][0][0],
                                          L.u, L.gm, r);
    loop_gmax_out(c, L.gm);
}
