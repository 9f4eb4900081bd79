// Definitions with no HIP dependency, shared by the kernels (through common.h) and by the host-only launch-plan code
// (igemm_plan.h), which the plain host compiler builds.
#pragma once
#include <stdint.h>
#include "../../include/mmvqa.h"

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_SERF = 3, ACT_SILU = 4, ACT_SIGMOID = 5 };
// A/B operand prologues (applied when a tile is written to LDS)
enum { PRO_NONE = 0, PRO_AFFINE_RELU = 1, PRO_DZ = 2, PRO_AFFINE = 3, PRO_AFFINE_SILU = 4, PRO_SILU_GATE = 5 };
// epilogue special modes
enum { EPI_PLAIN = 0, EPI_TAP_FWD = 1, EPI_TAP_BWD = 2 };
// contraction kinds of the implicit-GEMM family (MMVQA_KIND_* in the ABI)
enum { KIND_FWD = 0, KIND_DGRAD = 1, KIND_WGRAD = 2 };

typedef mmvqa_gemm_desc GemmParams;
typedef mmvqa_bn_fold BnFold;

int mmvqa_set_error(int code, const char* fmt, ...);
const char* mmvqa_get_error();
#define MMVQA_OK 0
#define MMVQA_ERR_ARG -1
#define MMVQA_ERR_HIP -2
#define MMVQA_ERR_STATE -3
