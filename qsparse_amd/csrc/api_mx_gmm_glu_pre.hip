// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the grouped gated matrix product on MX codes that also keeps its
// pre-activations (qs_mx_glu.h, PRE = true): the kernels of api_mx_gmm_glu.hip with one more output, v [T, 2 H] = accumulator + bias
// rounded once, +0 in the tail rows.  Instantiations of their own: the kernels of api_mx_gmm_glu.hip are not touched by them.
// Host side: argument checks, route, launch configuration (qs_mx_glu.h).  No allocation, no synchronisation, no read of offs.
#include "qs_mx_glu.h"

extern "C" {

int qs_mx_grouped_glu_matmul_pre_route(const qs_mx_grouped_glu_matmul_args* args) {
    qs_mx_grouped_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_gmm_glu_route(a, true);
}

int qs_mx_grouped_glu_matmul_pre_v(const qs_mx_grouped_glu_matmul_args* args) {
    qs_mx_grouped_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_gmm_glu_route(a, true);
    if (route <= 0) return route;
    return mx_gmm_glu_launch<true>(a, route);
}

}  // extern "C"
