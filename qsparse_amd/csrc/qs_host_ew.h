// Launch plan of the element-wise kernels (qs_elementwise.h): geometry + channel mode, kernel choice.
#pragma once
#include "qs_host.h"
#include "qs_elementwise.h"

namespace {

// geometry + channel mode of an element-wise launch over [outer, C, inner]
struct EwPlan {
    EwGeom geo;
    int cm;
};

// `last_ok`: the caller's parameter is tensor-wise and its channel mask (if any) is 8-byte aligned, so that a tensor
// whose channel dim is the innermost one (channels_last activations: outer = N*H*W, inner = 1) may take CM_LAST
int plan_ew(int64_t outer, int64_t C, int64_t inner, bool per_channel, EwPlan* plan, bool last_ok = false) {
    if (outer < 0 || C < 1 || inner < 1) return QS_ERR_ARG;
    const int64_t numel = outer * C * inner;
    if (numel / 8 >= ((int64_t)1 << 32) || C >= ((int64_t)1 << 32) || inner >= ((int64_t)1 << 32)) return QS_ERR_ARG;
    plan->geo.numel = numel;
    plan->geo.ngroups = numel / 8;
    plan->geo.C = (uint32_t)C;
    plan->geo.inner = (uint32_t)inner;
    plan->geo.groups_per_row = (uint32_t)(inner / 8);
    plan->geo.reverse = ew_reverse() ? 1u : 0u;
    if (!per_channel) plan->cm = CM_SCALAR;
    else if (inner % 8 == 0) plan->cm = CM_ROW;
    else if (last_ok && inner == 1 && C % 8 == 0) plan->cm = CM_LAST;
    else plan->cm = CM_ELEM;
    return QS_OK;
}

inline int ew_widen() {
    static int v = env_int("QS_EW_WIDEN", 2);
    return v;
}

// the channel mode of a kernel whose lanes take 4 elements at a time (the widening kernel, the STE backward): rows of 4k
// elements -- 14x14 maps -- keep one channel per lane there as well
inline int cm_4(const EwPlan& plan) { return plan.cm == CM_ELEM && plan.geo.inner % 4 == 0 ? CM_ROW : plan.cm; }

// the kernel a forward launch takes: the widening one (float32 output, no codes, a 4-per-lane channel mode; QS_EW_WIDEN:
// 0 off, 1 two-byte inputs only, 2 (default) fp32 inputs as well) in its channel mode, or else the 8-per-lane one in the plan's
struct EwRoute {
    bool widen;
    int cm;
};
inline EwRoute ew_route(const EwPlan& plan, int xdt, int ydt, bool codes) {
    const int cm4 = cm_4(plan);
    if (ydt == QS_F32 && ew_widen() >= (xdt == QS_F32 ? 2 : 1) && !codes && cm4 != CM_ELEM) return {true, cm4};
    return {false, plan.cm};
}

// channel mode -> compile-time constant (as with_dtype)
template <typename F>
int with_cm(int cm, F&& f) {
    switch (cm) {
        case CM_SCALAR: return f(IC<CM_SCALAR>{});
        case CM_ROW: return f(IC<CM_ROW>{});
        case CM_LAST: return f(IC<CM_LAST>{});
    }
    return f(IC<CM_ELEM>{});
}

// `elide`: skip the loads of lanes whose elements are all pruned (qs_elementwise.h, "Mask-aware traffic elision");
// only meaningful for ops that carry a channel mask, in the per-channel modes
template <typename Op, int XDT, int YDT, bool ELIDE>
int launch_ew_impl(const Op& op, const EwPlan& plan, bool param_per_channel, const void* x, void* y, int32_t* codes,
                   hipStream_t s) {
    constexpr bool NT = QS_EW_NT != 0;
    const EwRoute r = ew_route(plan, XDT, YDT, codes != nullptr);
    return with_cm(r.cm, [&](auto M) {
        constexpr int CM = decltype(M)::value;
        auto go = [&](auto P) {
            constexpr bool PPC = decltype(P)::value;
            if constexpr (YDT == QS_F32 && CM != CM_ELEM) {
                if (r.widen) {
                    const int64_t waves = (plan.geo.ngroups * 8 + 511) / 512;
                    const int gridw = (int)std::max<int64_t>(1, (waves + kWidenBlock / 64 - 1) / (kWidenBlock / 64));   // < 8 elements: tail only
                    hipLaunchKernelGGL((ew_widen_kernel<Op, XDT, CM, PPC, NT, ELIDE>), dim3(gridw), dim3(kWidenBlock), 0, s, op,
                                       plan.geo, x, (float*)y);
                    return launch_status();
                }
            }
            constexpr int U =   // groups per lane
                CM == CM_ELEM ? 1 : ELIDE ? QS_EW_UNROLL_ELIDE : CM == CM_SCALAR ? QS_EW_UNROLL_SCALAR : CM == CM_ROW ? QS_EW_UNROLL_ROW : QS_EW_UNROLL;
            hipLaunchKernelGGL((ew_kernel<Op, XDT, YDT, CM, PPC, NT, U, ELIDE>), dim3(grid_for(plan.geo.ngroups, U)), dim3(kBlock),
                               0, s, op, plan.geo, x, y, codes);
            return launch_status();
        };
        if constexpr (ELIDE && CM == CM_SCALAR) return launch_status();   // (never asked: launch_ew elides per channel only)
        else if constexpr (CM == CM_ROW || CM == CM_ELEM) return param_per_channel ? go(std::true_type{}) : go(std::false_type{});
        else return go(std::false_type{});
    });
}

template <typename Op, int XDT, int YDT>
int launch_ew(const Op& op, const EwPlan& plan, bool param_per_channel, const void* x, void* y, int32_t* codes,
              hipStream_t s, bool elide = false) {
    if (plan.geo.numel == 0) return QS_OK;
    if constexpr (Op::kHasMask && !OpGate<Op>::value) {     // (a gate-recording op loads every element: no elision)
        if (elide && plan.cm != CM_SCALAR && op.mask_ptr() != nullptr)
            return launch_ew_impl<Op, XDT, YDT, true>(op, plan, param_per_channel, x, y, codes, s);
    }
    return launch_ew_impl<Op, XDT, YDT, false>(op, plan, param_per_channel, x, y, codes, s);
}

int check_param(const float* p, int64_t nparam, int64_t C) {
    if (p == nullptr) return nparam == 1 ? QS_OK : QS_ERR_ARG;
    if (nparam != 1 && nparam != C) return QS_ERR_ARG;
    return QS_OK;
}

// the argument checks shared by the STE backward's two front ends (api_quant_bwd.hip: the ReLU family, or its gate bitmap;
// api_quant_bwd_act.hip: the caller's activation at act_x) and the plan of their launch.  `x` is the input the backward reads,
// `gate` the bitmap that may replace it; `g2_gate`: a second gradient stream (g2) is served by the gate bitmap kernels only.
// QS_OK with plan->geo.numel == 0: nothing to launch.
inline int ste_bwd_check(const qs_ste_relu_bwd_args& a, const void* x, const uint8_t* gate, bool g2_gate, EwPlan* plan) {
    if ((!a.g && !a.g2) || (!x && !gate) || !a.gx) return QS_ERR_ARG;
    if (!dt_ok(a.gdt) || !dt_ok(a.xdt) || !(a.gdt == QS_F32 || a.gdt == a.xdt)) return QS_ERR_DTYPE;
    if (a.g2 && ((g2_gate && !gate) || a.gdt != QS_F32 || (a.g2dt != QS_BF16 && a.g2dt != QS_F16))) return QS_ERR_DTYPE;
    if ((a.g && !aligned16(a.g)) || (!gate && !aligned16(x)) || !aligned16(a.gx) || (a.g2 && !aligned16(a.g2))) return QS_ERR_ALIGN;
    // the riders of the all-fp32 kernel form (BwdRiders, qs_elementwise.h)
    if (a.g3 && (!a.g2 || a.gdt != QS_F32 || a.xdt != QS_F32)) return QS_ERR_ARG;
    if (a.gx_image && (a.gdt != QS_F32 || a.xdt != QS_F32 || (a.gx_image_dt != QS_BF16 && a.gx_image_dt != QS_F16))) return QS_ERR_DTYPE;
    if ((a.g3 && !aligned16(a.g3)) || (a.gx_image && !aligned16(a.gx_image))) return QS_ERR_ALIGN;
    const int st = check_param(a.step, a.nstep, a.C);
    if (st) return st;
    const bool ppc = a.nstep > 1;
    return plan_ew(a.outer, a.C, a.inner, ppc || a.chan_mask != nullptr, plan, !ppc && aligned8(a.chan_mask));
}

}  // namespace

namespace {
// (shared by the forward units api_quant_fwd.hip / api_quant_fwd2.hip)
// the image of a quantizer's float32 output is written by the gate-recording widening kernels only (ew_widen_kernel<GateOp<..>>),
// so it needs a gate bitmap and the widening route (ew_route) for the launch's plan (the same kernels write relu(x) back: xback_out)
inline bool widen_route_ok(int64_t outer, int64_t C, int64_t inner, bool ppc, const uint8_t* chan_mask, const int32_t* codes,
                    const uint8_t* gate_out, int xdt, int ydt) {
    EwPlan plan;
    return gate_out && plan_ew(outer, C, inner, ppc || chan_mask != nullptr, &plan, !ppc && aligned8(chan_mask)) == QS_OK &&
           ew_route(plan, xdt, ydt, codes != nullptr).widen;
}
inline bool image_route_ok(int64_t outer, int64_t C, int64_t inner, bool ppc, const uint8_t* chan_mask, const int32_t* codes,
                    const uint8_t* gate_out, int xdt, int ydt, int imgdt, const void* image_out) {
    if ((imgdt != QS_BF16 && imgdt != QS_F16) || !aligned16(image_out)) return false;
    return widen_route_ok(outer, C, inner, ppc, chan_mask, codes, gate_out, xdt, ydt);
}
}  // namespace
