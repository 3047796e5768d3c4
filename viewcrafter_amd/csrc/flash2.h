// Interface between attention.hip (C ABI entry, dispatch) and attention_v2.hip (software-pipelined flash kernel).
#pragma once
#include "attn_mx.h"      // (-> mx_format.h -> vcx_common.h)

struct Flash2Args {
    const half_t* q;
    const half_t* k;
    const half_t* vt;
    half_t* o;
    int heads, nq, nk, kv_rows, kv_div;
    int64_t ldq, ldk, ldvt, ldo;
    vcxmx::AttnMxOut mx;   // mx.q != nullptr: the MXQ instantiation writes quant(o with ldo = 64 heads) here and o is not touched
    int nqb, nprob;   // 256-row query blocks per problem, problems (group x head): 1-D grid of nqb * roundup(nprob, 8)
};

// nk % 64 == 0, base-2 logits (VCX_ATTN_LOG2_LOGITS), no accumulate: checked by the caller.
int vcx_flash2_launch(const Flash2Args& a, hipStream_t s);
