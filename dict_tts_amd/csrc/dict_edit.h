// Editing the resident dictionary table in place (dict_edit.hip; dtts_text2mel_fetch(DTTS_DICT_EDIT / DTTS_DICT_ENTRY)): replace and append
// entries of the table of dtts_dict_table_upload (text2mel.hip) so that it equals, bit for bit, a fresh upload of the edited dictionary.
// Entry order is kept, so the entries between two edited ones are ONE contiguous run of rows in the old and in the new table: a whole array
// moves as at most 2 n_edit + 1 contiguous segments, each from the old array or from the staging array of the new entries' rows, and one
// launch of the segment-copy kernel moves them all.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dicttts_hip.h"

namespace dtts {

// One contiguous run, in ROWS of the array it is applied to (gloss rows for K / V / key_map, pinyin slots for pinyin / pinyin_map).  A list
// is sorted by dst, has no empty segment and covers the new array's rows 0 .. total - 1 exactly once
struct DictSeg {
    int dst;      // first row in the new array
    int src;      // first row in the source
    int rows;     // > 0
    int staged;   // 0: the source is the old array, 1: the staging array of the edited entries
};

constexpr int DICT_SEG_UNROLL = 4;                       // elements in flight per lane
constexpr int DICT_SEG_TILE = 256 * DICT_SEG_UNROLL;     // consecutive elements of the new array per workgroup

// new_[r] = (staged ? staging : old)[...] for every row r of every segment, in ONE launch whatever n_seg is.  elem_bytes 16 / 8 / 4 = the
// instantiation (a row is `width` such elements: hidden_size / 4 for the K / V rows, 1 for the others); the pointers are aligned to
// elem_bytes.  segs_dev [n_seg] lives on the device.  total_rows = 0 (or n_seg = 0) launches nothing.  hipErrorInvalidValue for another
// elem_bytes
hipError_t dict_seg_copy_launch(int elem_bytes, const void* old, const void* staging, void* new_, const DictSeg* segs_dev, int n_seg, int width,
                                long long total_rows, hipStream_t stream);

} // namespace dtts
