// Host side of the paired backward launch: the dgrad + wgrad entry points run a layer's input gradient and
// its weight gradient through ONE main launch where both land on kernels with a paired form.  While such a call dispatches its
// input gradient (`collect`), a launcher of one of those kernels does not launch: it hands its plan to the stash below.  The
// weight gradient that follows takes it into its own launch (igemm2_pair, kpair_k, linear_bwd_k); any other kernel leaves it to be
// launched on its own (flush).  Host only, and included below the three kernel families because it holds their plans; their
// launchers reach it through pair_collecting / pair_stash / pair_flush, declared in front of them.
#pragma once

struct PairStash {
    enum Kind { NONE, TILE, KGEMM, LINEAR };
    bool collect = false;
    Kind kind = NONE;     // which input gradient waits, and its plan:
    v2::TileDgrad tile;   // igemm_v2.h, FWD or BWD gather form on a small tile, with its split-K finish
    kg::KDgrad k;         // kgemm.h
    lin::LinProb lin;     // linear_small.h
    size_t ws_used = 0;   // bytes of the call's scratch arena the waiting plan occupies (the tiled plan's slabs)
    bool paired = false;  // out: the two went out as one kernel

    void clear() { collect = false, kind = NONE, ws_used = 0, paired = false; }
    void put(const v2::TileDgrad& p) { kind = TILE, tile = p, ws_used = p.slab_bytes; }
    void put(const kg::KDgrad& p) { kind = KGEMM, k = p, ws_used = 0; }
    void put(const lin::LinProb& p) { kind = LINEAR, lin = p, ws_used = 0; }
    int flush(hipStream_t st) {  // whatever waits goes on its own
        const Kind was = kind;
        kind = NONE, ws_used = 0;
        if (was == TILE) return v2::launch_tile_dgrad(tile, st);
        if (was == KGEMM) return kg::launch_kdgrad(k, st);
        if (was == LINEAR) return lin::launch_linear_dgrad(lin, st);
        return MOVAE_OK;
    }
};
static thread_local PairStash g_stash;

inline bool pair_collecting() { return g_stash.collect; }
template <class Plan>
inline void pair_stash(const Plan& p) { g_stash.put(p); }
inline int pair_flush(hipStream_t st) { return g_stash.flush(st); }

// The tiled weight gradient (plan: v2::plan_wgrad2), launched with the stashed input gradient of its layer where the two pair
template <int BM, int BN>
int launch_wgrad2(const float* Sm, const float* Bg, float* const* dW, int G, long s_gs, long b_gs, const WGeom& g, int K,
                  int accumulate, void* ws, size_t ws_bytes, hipStream_t st, float* const* colsum = nullptr) {
    v2::WgPlan w;
    if (int rc = v2::plan_wgrad2(BM, BN, Sm, Bg, dW, G, s_gs, b_gs, g, K, accumulate, ws, ws_bytes, colsum, &w)) return rc;
    PairStash& s = g_stash;
    const v2::TileDgrad& p = s.tile;
    if (s.kind == PairStash::KGEMM && v2::pair_wgrad_tile<BM, BN>()) {
        s.kind = PairStash::NONE, s.paired = true;
        if (int rc = kg::launch_kpair(s.k, w.a, w.gx, w.gy, w.gz, BM == 64, st)) return rc;
    } else if (s.kind == PairStash::TILE && v2::pair_wgrad_tile<BM, BN>() &&
               (long)p.gx * p.gy * p.gz + (long)w.gx * w.gy * w.gz < 0x7fffffffL) {
        s.kind = PairStash::NONE, s.paired = true;
        constexpr int W64 = BM == 64 ? 1 : 0;  // wgrad tile: <64,64> or <32,128>
        // names as rocprofv3 prints the instantiations: <form, dgrad tile, wgrad tile>
        if (p.form == 0 && p.bm == 64) {
            v2::launch_pair<0, 64, 64, W64 ? 64 : 32, W64 ? 64 : 128>(p, w.a, w.gx, w.gy, w.gz, st);
            g_last_kernel = W64 ? "igemm2_pair<0,64,64,64,64>" : "igemm2_pair<0,64,64,32,128>";
        } else if (p.form == 0) {
            v2::launch_pair<0, 128, 32, W64 ? 64 : 32, W64 ? 64 : 128>(p, w.a, w.gx, w.gy, w.gz, st);
            g_last_kernel = W64 ? "igemm2_pair<0,128,32,64,64>" : "igemm2_pair<0,128,32,32,128>";
        } else if (p.bm == 64) {
            v2::launch_pair<1, 64, 64, W64 ? 64 : 32, W64 ? 64 : 128>(p, w.a, w.gx, w.gy, w.gz, st);
            g_last_kernel = W64 ? "igemm2_pair<1,64,64,64,64>" : "igemm2_pair<1,64,64,32,128>";
        } else {
            v2::launch_pair<1, 128, 32, W64 ? 64 : 32, W64 ? 64 : 128>(p, w.a, w.gx, w.gy, w.gz, st);
            g_last_kernel = W64 ? "igemm2_pair<1,128,32,64,64>" : "igemm2_pair<1,128,32,32,128>";
        }
        MOVAE_CHECK_LAUNCH("igemm2_pair");
        if (int rc = v2::finish_tile_dgrad(p, st)) return rc;
    } else {
        if (int rc = s.flush(st)) return rc;
        dim3 grid(w.gx, w.gy, w.gz);
        int gz;
        const RSide sd = defer_take_3d(st, &grid, &gz);
        if (BM == 128 && BN == 128 && g_movae_compute_bf16) hipLaunchKernelGGL((v2::igemm2_wgrad<BM, BN, BM == 128 && BN == 128>), grid, dim3(256), 0, st, w.a, sd, gz);
        else hipLaunchKernelGGL((v2::igemm2_wgrad<BM, BN>), grid, dim3(256), 0, st, w.a, sd, gz);
        MOVAE_CHECK_LAUNCH("igemm2_wgrad");
    }
    return v2::reduce_wgrad2(w, dW, G, accumulate, st, colsum);
}
