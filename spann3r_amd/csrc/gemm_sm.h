// Internal interface between sp3_gemm's dispatcher (gemm.hip) and the lean small-M instances (gemm_sm.hip).
#pragma once
#include "common.h"

// tile id (>= 30) of the lean instance that serves this (validated) descriptor, or -1
int sp3_gemm_sm_tile(const sp3_gemm_desc& d);
// true if that instance also serves PAIRED launches (sp3_gemm_n, n = 2): the q/k/v projections' ROPE instances only
bool sp3_gemm_sm_pairs(const sp3_gemm_desc& d);
// launches d (and, in the same launch, `pair` if non-null) on its lean instance; 0 on success
int sp3_gemm_sm_launch(const sp3_gemm_desc& d, const sp3_gemm_desc* pair, hipStream_t stream);
// true if the n (2..4) validated descriptors are all small-map convolutions of one map dtype (tiles 40 / 41, mixed): sp3_gemm_n sends
// them as one level launch (the level kernel holds tile 41 for bf16 maps only: an fp32 map on tile 41 goes out on its own first)
bool sp3_gemm_sm_conv_level(const sp3_gemm_desc* ds, int n);
int sp3_gemm_sm_conv_level_launch(const sp3_gemm_desc* ds, int n, hipStream_t stream);
