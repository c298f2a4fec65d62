// csrc/ac_device_dec.hip for the decoder scales of csrc/decode.hip (C++ linkage, not exported): the parts of linr_rc_decode_probs,
// so that a scale checks and uploads the entries of its 8 stages once and launches rc_decode_k per stage on a slice of the table.
#pragma once
#include "common.h"

// the whole table against the sizes of its buffers, output row ranges that overlap included: 0 or LINR_EINVAL; launches nothing
__attribute__((visibility("hidden")))
int linr_rc_dec_check(const linr_rc_dec_entry* e, int32_t n_entries, int64_t n_probs, int64_t bytes_len, int64_t n_rows);
// the table to tab_dev as kernel arguments: the host array is free on return
__attribute__((visibility("hidden")))
int linr_rc_dec_upload(const linr_rc_dec_entry* e, int32_t n_entries, linr_rc_dec_entry* tab_dev, hipStream_t s);
// rc_decode_k over n_entries entries of a checked table (0: nothing); bytes_dev: 4-byte aligned, readable up to its length rounded up to 4
__attribute__((visibility("hidden")))
int linr_rc_dec_launch(const float* probs, const uint8_t* bytes_dev, const linr_rc_dec_entry* tab_dev, int32_t n_entries, float* occ_col,
                       int64_t occ_ld, uint8_t* sym_dev, hipStream_t s);
