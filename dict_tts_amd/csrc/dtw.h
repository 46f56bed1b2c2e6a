// Dynamic time warping of a batch of sequence pairs (dtw.hip; dtts_text2mel_fetch(DTTS_OUT_DTW)): the reference's utils/dtw.py::dtw with
// the cost |x - y| (scripts/pitch_dtw.py), accelerated_dtw with the cityblock cost, _traceback, and the F0 moments pitch_dtw.py prints.
// One add of an exact minimum per cell: every schedule gives the reference's bits.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dicttts_hip.h"

namespace dtts {

constexpr int DTW_LANE_ROWS = 16;                      // rows a lane owns: their 2-bit direction codes fill one dword per column
constexpr int DTW_STRIP_ROWS = DTTS_DTW_STRIP_ROWS;    // 64 lanes of them
constexpr int DTW_MAX_LEN = DTTS_DTW_MAX_LEN;
constexpr int DTW_MAX_F = 128;
static_assert(DTW_STRIP_ROWS == 64 * DTW_LANE_ROWS, "a strip is one wave of lanes");

// where the forward kernel takes a cell's cost from
enum { DTW_COST_F32 = 0, DTW_COST_F64 = 1, DTW_COST_WS = 2 };

struct DtwParams {
    const void* x;            // [B][x_ld][F]
    const void* y;            // [B][y_ld][F]
    const int* x_lens;        // [B] or null
    const int* y_lens;        // [B] or null
    double* dist;             // [B]
    int* path;                // [B][2][path_ld] or null
    int* path_len;            // [B]
    double* acc;              // [B][x_ld][y_ld] or null
    double* moments;          // [B][2][4] or null
    unsigned* dirs;           // workspace [B][dir_stride]: a pair's codes as [strip][k][lane], k = column + lane in 0 .. M + 62; or null
    const double* cost;       // workspace [B][cost_stride]: a pair's costs as [strip][k][r][lane] (F > 1), or null
    double* cost_w;           //   the same, for the launch that fills it
    size_t dir_stride, cost_stride;
    double slope;
    int B, F, x_ld, y_ld, window, path_ld;   // window < 0: no band
};

inline int dtw_strips(int rows) { return (rows + DTW_STRIP_ROWS - 1) / DTW_STRIP_ROWS; }
// the skewed column index k = j + lane runs over y_ld + 63 values per strip
inline size_t dtw_dir_words(int x_ld, int y_ld) { return (size_t)dtw_strips(x_ld) * (size_t)(y_ld + 63) * 64; }
inline size_t dtw_cost_words(int x_ld, int y_ld) { return dtw_dir_words(x_ld, y_ld) * DTW_LANE_ROWS; }
// LDS of the forward launch: the last row of a strip, read by the next one (nothing for a single strip)
inline size_t dtw_lds_bytes(int x_ld, int y_ld) { return x_ld > DTW_STRIP_ROWS ? (size_t)y_ld * sizeof(double) : 0; }

hipError_t dtw_cost_launch(const DtwParams& p, int dtype, hipStream_t stream);
hipError_t dtw_forward_launch(const DtwParams& p, int mode, hipStream_t stream);
hipError_t dtw_path_launch(const DtwParams& p, hipStream_t stream);

} // namespace dtts
