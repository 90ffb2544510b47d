// vibo_variant.hpp -- which instantiation of the row-split ELBO kernels a launch runs, and the rules that follow from that choice: ONE
// definition for the kernels' own constants (vibo_msplit_kernel.hpp, vibo_helpers.hip), the host dispatch (split_variant, launch_split) and
// the folded step's contract (step_contract).  Plain constexpr functions and PODs for host and device code: no HIP runtime calls.
#pragma once

namespace vibo {

// which row-split kernel (Panels / Split): vibo_split_kernel.hpp | vibo_msplit_kernel.hpp | vibo_narrow.hip (<= 128 items, a row per 16 lanes)
enum class Engine { Valu, Matrix, Narrow };
// the kernels' template parameter RM: how the rows reach the kernel
enum RowMode : int {
    kRowsInOrder = 0,    // fp32 responses + mask bytes (or no mask), rows in order
    kRowsGathered = 1,   // the same through row_index
    kRowsCodes = 2,      // 1-byte cell codes (VIBO_MASK_CODES), with or without row_index
    kRowsSign = 3,       // fp32 responses in order whose sign bit is the mask (VIBO_MASK_SIGN): matrix kernel, no hooks, no flows
    kRowsTiles = 4       // the matrix' prepacked code words and counts (VIBO_MASK_TILES, include/vibo_hip_tile_rows.h): the same launches,
                         // and hook mode kHooksGiven without flows (include/vibo_hip_given_tiles.h)
};
// VIBO_MASK_TILES: bytes of one wave's block of the image (16 code words and one counts dword per lane), and of its code words
constexpr int kTileWaveBytes = 4352, kTileWordBytes = 4096;
// the matrix kernel's template parameter XM: which hooks the launch uses (the VALU kernel reads the same fields at run time)
enum HookMode : int {
    kHooksNone = 0,
    kHooksPanel = 1,     // panel / conditional: row_cnt, pre_stats, post_coef, primary == 0, panel_count
    kHooksGiven = 2,     // caller-supplied posterior read / written by the slot lanes: given_post, given_grad (one panel)
    kHooksCondFused = 3  // conditional posterior with the experts' sums formed in the kernel: cond_table, codes_out, post_coef
};
struct SplitVariant {
    Engine engine;
    int at;              // template ability width: 2 / 4 / 8 (Valu), 8 (Matrix), 1 / 2 / 4 (Narrow)
    int irt;             // 1 / 2 / 3 PL
    bool grad, flows;
    int rm, xm;          // RowMode, HookMode
    int waves;           // per workgroup: nw = ceil(items / 128) (Matrix), nq = ceil(items / 256) (Valu), 4 (Narrow)
    bool nw8;            // Matrix: exactly 8 waves
};
constexpr bool ms_may_gather(int rm) { return rm == kRowsGathered || rm == kRowsCodes; }      // the instantiation can meet row_index
// the matrix kernel draws the ability noise itself where the launch passes no eps (the folded train step)
constexpr bool ms_draws_noise(int xm, bool flows, bool grad) { return xm == kHooksNone && !flows && grad; }
// ... and such a launch may pass no `ability` either: the <fp32 rows gathered, fewer than 8 waves> instantiations store the sample
// unconditionally (they measured slower with the choice than with the store)
constexpr bool ms_sample_optional(int xm, bool flows, bool grad, int rm, bool nw8) {
    return ms_draws_noise(xm, flows, grad) && (nw8 || rm != kRowsGathered);
}
// the matrix kernel's batch loop with ONE workgroup barrier per batch (the per-person phase of the neighbouring batches runs under the
// SIMD partner's tiles): tile rows at exactly 8 waves -- their counts are data of the image, requested two batches ahead.  (Tile rows
// under a caller-supplied posterior, kHooksGiven, keep the two-barrier loop at every width.)
constexpr bool ms_one_barrier(int rm, int xm, bool flows, bool nw8) { return rm == kRowsTiles && xm == kHooksNone && !flows && nw8; }
// ... and with the (person, dim) chains on four waves of their own, one per SIMD beside the eight tile waves (a third wave per SIMD:
// at most 168 registers): the one-barrier instantiations with gradients, 1PL / 2PL.  (3PL holds 204 registers without the chains;
// a forward-only launch has no backward chain to move.)  ONE definition for the kernel's constant, its launch bounds and the
// launch's block size.
constexpr bool ms_chain_waves(int irt, bool grad, int rm, int xm, bool flows, bool nw8) {
    return ms_one_barrier(rm, xm, flows, nw8) && grad && irt != 3;
}
constexpr int kMsChainWaves = 4;
// threads of a matrix-kernel workgroup of nw (tile) waves, and the waves per SIMD the instantiation is compiled for
constexpr int ms_block_threads(int nw, bool chain_waves) { return 64 * (nw + (chain_waves ? kMsChainWaves : 0)); }
constexpr int ms_waves_per_simd(bool chain_waves) { return chain_waves ? 3 : 2; }
// the matrix kernel keeps a batch's code words PAIRED in registers (words k and k + 1 of a lane byte-interleaved where they become the
// current batch's, so that a tile converts cells k and k + 1 of ITSELF into adjacent registers), sums the d LL/d theta shares with one
// DPP add per value and lays the tile's clamp path out of line: every tile-rows instantiation.  The image in memory is not affected.
constexpr bool ms_word_pairs(int rm) { return rm == kRowsTiles; }
constexpr bool ms_draws_noise(const SplitVariant& v) { return v.engine == Engine::Matrix && ms_draws_noise(v.xm, v.flows, v.grad); }
constexpr bool ms_sample_optional(const SplitVariant& v) {
    return v.engine == Engine::Matrix && ms_sample_optional(v.xm, v.flows, v.grad, v.rm, v.nw8);
}
// outputs per workgroup of the finalize (finalize_kernel's template parameter) over n_out outputs and bpp partial records per panel:
// many small records, or the few outputs of a forward-only call, get more slices per output
constexpr int finalize_group(int bpp, int n_out) { return (bpp >= 1024 || n_out <= 64) ? 16 : 64; }

}  // namespace vibo
