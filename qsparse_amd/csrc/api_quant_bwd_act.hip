// libqsparse_hip.so -- the STE backward with the CALLER'S activation's backward on the way out (qs_ste_relu_bwd_args::act_x,
// ABI v26; ste_relu_bwd_kernel<..., DACT>).  A translation unit of its own: its kernel instantiations compile next to the others.
#include "qs_host_ew.h"

// called by qs_quant_ste_relu_bwd_v (api_quant_bwd.hip) when the descriptor names an act_x; arguments already copied
int qs_ste_act_bwd_impl(const qs_ste_relu_bwd_args& a) {
    if (a.act_x_kind != QS_DACT_GELU) return QS_ERR_ARG;
    EwPlan plan;
    const int st = ste_bwd_check(a, a.act_x, nullptr, false, &plan);
    if (st || plan.geo.numel == 0) return st;
    const bool ppc = a.nstep > 1;
    hipStream_t s = (hipStream_t)a.stream;
    SteBwdOp op{a.step, a.step_host, a.step_is_decimal, a.lo_mul, a.hi_mul, 0, a.chan_mask};
    const BwdRiders rd{a.g3, a.gx_image, a.gx_image_dt};
    const int grid = grid_for(plan.geo.ngroups, 1);
    constexpr bool NT = QS_EW_NT != 0;
    const ActSpec act{QS_ACT_NONE, 0.f, 0.f};
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        auto go = [&](auto G, auto G2) {
            constexpr int GD = decltype(G)::value, G2D = decltype(G2)::value;
            return with_cm(GD == QS_F32 && XD == QS_F32 ? cm_4(plan) : plan.cm, [&](auto M) {
                hipLaunchKernelGGL((ste_relu_bwd_kernel<GD, XD, decltype(M)::value, NT, false, false, G2D, QS_DACT_GELU>), dim3(grid),
                                   dim3(kBlock), 0, s, op, plan.geo, (int)ppc, a.g, a.act_x, a.gx, act, a.g2, rd);
                return launch_status();
            });
        };
        if (a.g2) return a.g2dt == QS_BF16 ? go(IC<QS_F32>{}, IC<QS_BF16>{}) : go(IC<QS_F32>{}, IC<QS_F16>{});
        return a.gdt == QS_F32 ? go(IC<QS_F32>{}, IC<-1>{}) : go(X, IC<-1>{});
    });
}
