// attract.hpp -- the attraction of the gradient (attract.hip): the tiled and
// stream layouts of a rank's rows of P, and the launches over them or over
// the CSR rows.  Internal to the optimizer (optimize.hip).
#pragma once
#include <cstdlib>

#include "common.hpp"

namespace tsne {

// one tile of the tiled attraction (attract_tiles): the entries of a row
// block whose column lies in one window of labels, as 64-row slices
struct ATile {
    int32_t s0;    // first slice
    int32_t ns;    // slices
    int32_t cb;    // column window
    int32_t rb;    // row block
};
struct ASlice {
    int64_t base;    // first entry (step 0, lane 0)
    int32_t width;   // steps: entries of the slice's first (longest) lane
    int32_t wide;    // 1: one long row split over the 64 lanes (wave-reduced)
    int32_t j0;      // first (sorted) segment
    int32_t cnt;     // segments (rows): <= 64, or 1 for a wide slice
};

struct AWave {       // stream layout (attract_tiles_stream): a wave's share of a row block
    int32_t q0;      // its first slice in the dealt list
    int32_t cnt;     // its slices
    int32_t steps;   // the sum of their widths
    int32_t g0;      // its stream's first group
};

struct AttractLayout {
    // tiled attraction layout of the owned rows (attract_tiles), rebuilt with them
    bool at_on = false;
    int64_t at_nrb = 0, at_ncb = 0;
    int64_t at_rbs = 0;       // rows per row block (<= the config's RB: the grid covers the CUs)
    int at_cfg = 0;
    int at_pipe = 0;   // Options::attract_pipe when the layout was built
    int at_dyn = 0;    // Options::attract_dyn
    ATile *at_tiles = nullptr;
    int32_t *at_rbt = nullptr;
    ASlice *at_slices = nullptr;
    uint32_t *at_srow = nullptr;
    uint16_t *at_pk = nullptr;
    double *at_pv = nullptr;
    // the stream layout of the same slices (attract_tiles_stream; Options::attract_stream)
    bool at_stream = false;
    int64_t at_pad_ppm = 0;   // its stored slots (64 per step) per real entry, in parts per million
    AWave *ats_waves = nullptr;
    int2 *ats_recs = nullptr;
    uint32_t *ats_lword = nullptr;
    uint8_t *ats_stream = nullptr;
};

// One attraction launch: the CSR rows [r0, r1) (rp indexed by label: rp[r0]
// is the first entry), the embedding, Z in scal[0] (loss launches), the sums
// (2-D) and the loss partials.
struct AttractArgs {
    const int64_t *rp; const int32_t *col; const double *val; int64_t r0, r1; const double *Y;
    const double *scal; int metric; double ex; double2 *attr; double *lpart;
    int bpc = 0;   // blocks per CU of the persistent grid (0: 8 = every wave slot)
    int64_t n = 0;   // points of Y (the tile kernels' last window ends there; attract_rows / attract3 ignore it)
};

// (Re)build `l` for the owned rows (rpw local: rpw[0] = 0) of an n-point,
// nnz-entry P with C components; off (l.at_on false) where attract_rows /
// attract3 are to run.  Synchronises the stream.
void attract_layout_build(tsne_ctx *ctx, AttractLayout &l, const int64_t *rpw, const int32_t *colw, const double *valw,
                          int64_t rows, int64_t n, int64_t nnz, int C, bool morton_labels);

// 2-D: attract_tiles (or its stream / pipe forms) over the layout when it is
// on, else attract_rows over the CSR rows (a default AttractLayout: no layout).
// 3-D: attract_tiles3 or attract3, the sums in attr3 (rows x 3; a.attr unused).
// Both return the blocks that wrote loss partials.
int64_t attract_launch_2d(hipStream_t st, const AttractLayout &l, const AttractArgs &a, bool loss);
int64_t attract_launch_3d(hipStream_t st, const AttractLayout &l, const AttractArgs &a, double *attr3, bool loss);

// upper bounds of the two launches' block counts over `rows` CSR rows (the loss partials' size)
int64_t attract_max_blocks(int64_t rows);
int64_t attract3_blocks(int64_t rows);

// TSNE_DEBUG_TILES=1: layout and per-iteration BH / tile diagnostics on stderr
// (synchronises; a debug print, no effect on results)
inline bool debug_tiles() {
    static const bool on = getenv("TSNE_DEBUG_TILES") != nullptr;
    return on;
}

}  // namespace tsne
