// Host side of the GEMM kernel families that live outside gemm.hip: a plain host entry per family, which picks its own template
// arguments (A mode / fast gather, GEGLU, causal) from the call; launch_route() in gemm.hip is the only caller.  What the launchers
// and the dispatch share lives here too.
#ifndef MOCA_GEMM_LAUNCH_H
#define MOCA_GEMM_LAUNCH_H
#include "gemm_device.h"

// gemm_tiled.hip: the 256 x BN direct-to-LDS kernel (bn = 128 or 160), g4,
int moca_gemm_glds_launch(int bn, const moca_gemm_params& p, hipStream_t st);
int moca_gemm_g4_launch(const moca_gemm_params& p, hipStream_t st);
// and the staggered kernel, shape = its SHAPE (0: 320 x 160, 1: 160 x 320, 2: 256 x 256, 3: 320 x 192 with temporal attention)
int moca_gemm_w80s_launch(int shape, const moca_gemm_params& p, hipStream_t st);
// gemm_halo.hip: the 320 x 160 staggered kernel with the LDS-resident halo tile (stride-1 3 x 3 convs, inW = 64 or 32)
int moca_gemm_w80h_launch(const moca_gemm_params& p, hipStream_t st);
// gemm_persistent.hip: g4p (g4q under MOCA_TUNE_GEMM_MF32) and sqp
int moca_gemm_g4p_launch(const moca_gemm_params& p, hipStream_t st);
int moca_gemm_sqp_launch(const moca_gemm_params& p, hipStream_t st);

namespace {

constexpr int G4P_BLOCKS = 512;                      // persistent two-blocks-per-CU kernel: two blocks on every CU
constexpr int SQP_BLOCKS = 256;                      // persistent 256 x 256 staggered kernel: one block on every CU

// XCD partition (xm x xn = 8, xn returned; 1 = the 1-D partition) of a tiles_m x tiles_n grid of row tiles x BN-column tiles of a LINEAR
// launch: estimated fabric bytes = W part + A part.  W: an XCD whose W sub-range ((tiles_n / xn) BN x K) fits its L2 (<= 3 MB)
// fetches it once -> xm |W| in total; one that does not streams it again for every M tile it owns -> tiles_m |W| whatever
// the partition.  A is consumed row tile by row tile -> xn |A|.  Only partitions that divide both tile counts; a 2-D partition is
// taken when it saves >= 20 %.
static int choose_xcd_n(const moca_gemm_params& p, int tiles_m, int tiles_n, int BN) {
    if (p.splits != 1 || p.a_mode != MOCA_A_LINEAR) return 1;
    const double Wtot = (double)p.N * p.K * 2, Atot = (double)p.M * p.K * 2;
    auto cost = [&](int xn) {
        const int xm = 8 / xn;
        const double wsub = (double)(tiles_n / xn) * BN * p.K * 2;
        return (wsub <= 3.6e6 ? xm * Wtot : tiles_m * Wtot) + xn * Atot;      // (3.3 MB of W + the A tiles in flight still mostly hit: -3..6 % on the 1280-channel GEGLU)
    };
    double best = cost(1);
    int best_xn = 1;
    for (int xn = 2; xn <= 8; xn *= 2) {
        if (tiles_m % (8 / xn) || tiles_n % xn) continue;
        const double c = cost(xn);
        if (c < 0.8 * best) { best = c; best_xn = xn; }
    }
    return best_xn;
}

inline bool fast_gather(const moca_gemm_params& p) {
    return (p.a_mode == MOCA_A_LINEAR) ? (p.K % BK == 0 && p.K <= 8192) : (p.C % BK == 0 && p.C <= 8192);
}
// a_mode / fast_gather as template arguments: f(int_c<AMODE>, yes_t / no_t)
template <typename F>
int with_gather(const moca_gemm_params& p, F f) {
    const bool fast = fast_gather(p);
    if (p.a_mode == MOCA_A_LINEAR) return fast ? f(int_c<MOCA_A_LINEAR>{}, yes_t{}) : f(int_c<MOCA_A_LINEAR>{}, no_t{});
    if (p.a_mode == MOCA_A_CONV3X3) return fast ? f(int_c<MOCA_A_CONV3X3>{}, yes_t{}) : f(int_c<MOCA_A_CONV3X3>{}, no_t{});
    return fast ? f(int_c<MOCA_A_TCONV3>{}, yes_t{}) : f(int_c<MOCA_A_TCONV3>{}, no_t{});
}

// a kernel's dynamic LDS limit, raised once per kernel instantiation (one flag per KERNEL); false: MOCA_E_LAUNCH
template <auto KERNEL>
bool dyn_lds_once(int lds) {
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return false;
        attr_set = true;
    }
    return true;
}

}  // namespace

#endif
