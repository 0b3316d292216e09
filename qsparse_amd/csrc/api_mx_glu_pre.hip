// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the gated matrix product on MX codes that also keeps its pre-activations
// (qs_mx_glu.h, PRE = true): the kernels of api_mx_glu.hip with one more output, v [M, 2 H] = accumulator + bias rounded once -- what a
// training step's backward reads.  Instantiations of their own: the kernels of api_mx_glu.hip are not touched by them.
// Host side: argument checks, route, launch configuration (qs_mx_glu.h).  No allocation, no synchronisation.
#include "qs_mx_glu.h"

extern "C" {

int qs_mx_glu_matmul_pre_route(const qs_mx_glu_matmul_args* args) {
    qs_mx_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_glu_route(a, true);
}

int qs_mx_glu_matmul_pre_v(const qs_mx_glu_matmul_args* args) {
    qs_mx_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_glu_route(a, true);
    if (route <= 0) return route;
    return mx_glu_launch<true>(a, route);
}

}  // extern "C"
