// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the gated matrix product on MX codes (qs_mx_glu.h): A . B^T on a weight of 2 H
// interleaved rows through the block-scaled MFMA, bias, act(gate) * up on the accumulators, then H columns as a float tensor or as MX
// codes, all 5 x 5 pairs of input formats; act and the output are kernel arguments.
// Host side: argument checks, route, launch configuration (qs_mx_glu.h, shared with api_mx_glu_pre.hip).  No allocation, no
// synchronisation.
#include "qs_mx_glu.h"

extern "C" {

int qs_mx_glu_matmul_route(const qs_mx_glu_matmul_args* args) {
    qs_mx_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_glu_route(a, false);
}

int qs_mx_glu_matmul_v(const qs_mx_glu_matmul_args* args) {
    qs_mx_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_glu_route(a, false);
    if (route <= 0) return route;
    return mx_glu_launch<false>(a, route);
}

}  // extern "C"
