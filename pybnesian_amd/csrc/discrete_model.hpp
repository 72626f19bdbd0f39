// The handle of a table of dictionary codes (pbn_dtable, discrete_model.hip), for the units that evaluate one: discrete_model.hip
// (pbn_dnet) and clg_model.hip (pbn_clgnet).
#pragma once
#include <cstdint>
#include <vector>

#include "common.hpp"
#include "scoring_internal.hpp"

struct pbn_dtable : pbn::score::FamilyScratch {
    pbn::ctx_ptr ctx;
    int64_t n_rows = 0;
    int n_cols = 0;
    std::vector<int> card;
    std::vector<std::vector<int32_t>> codes;   // host copy, source row order, -1 = null
    pbn::dev_buf<int32_t> codes_dev;           // [n_cols][n_rows]
    pbn::dev_buf<uint8_t> codes8;              // [n_cols][ld8], 0xFF = null and in the rows past the last
    int64_t ld8 = 0;                           // 0: no byte mirror
};
