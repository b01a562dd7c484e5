// include/cfen_padnorm.h: LayerNorm over token rows that carry padding slots.  The kernel is k_layernorm_padded of k_attention.hip, beside the
// k_layernorm it shares every line of arithmetic with (and that file's code generation flags); the launcher is the one the net's launch plan
// calls (cfen_net.cpp VitCtx::layernorm), so this entry point runs what a v5 forward runs.
#include "../../include/cfen_padnorm.h"
#include "cfen_common.hpp"
#include "cfen_internal.hpp"

extern "C" int cfen_layernorm_padded(int dtype, const void* X, void* Y, const float* gamma, const float* beta, int M, int D, int cs, int C, float eps,
                                     void* stream) {
  CFEN_CHECK_ARG(gamma && beta, "layernorm_padded: gamma/beta required");
  CFEN_CHECK_ARG(cs >= 1, "layernorm_padded: %d slots per pixel", cs);
  return cfen_layernorm_impl_g(dtype, 1, &X, &Y, &gamma, &beta, M, D, eps, (hipStream_t)stream, cs, C);
}
