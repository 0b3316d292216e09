// One wave, one v_mfma_scale_f32_16x16x128_f8f6f4, register images supplied by the host (tools/probes/probe_mfma_scale.py).
// Block p of the grid is problem p: lane l takes a[p][l][0..7], b[p][l][0..7], c[p][l][0..3], one scale dword per side, and
// writes d[p][l][0..3].  Formats and opsel are immediates of the instruction, hence the template and the switch.
//   hipcc --offload-arch=gfx950 -O2 -shared -fPIC tools/probes/probe_mfma_scale.hip -o tools/probes/libprobe_mfma_scale.so
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int FA, int FB, int OA, int OB>
__global__ __launch_bounds__(64) void probe_kernel(const int* a, const int* b, const float* c, const int* sa, const int* sb, float* d) {
    const int64_t l = (int64_t)blockIdx.x * 64 + threadIdx.x;
    i32x8 av, bv;
    f32x4 cv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        av[j] = a[l * 8 + j];
        bv[j] = b[l * 8 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cv[j] = c[l * 4 + j];
    const f32x4 r = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, cv, FA, FB, OA, sa[l], OB, sb[l]);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[l * 4 + j] = r[j];
}

template <int FA, int FB, int OA, int OB>
static int launch(int n, const int* a, const int* b, const float* c, const int* sa, const int* sb, float* d, hipStream_t s) {
    hipLaunchKernelGGL((probe_kernel<FA, FB, OA, OB>), dim3(n), dim3(64), 0, s, a, b, c, sa, sb, d);
    return (int)hipGetLastError();
}

template <int FA, int FB>
static int by_opsel(int oa, int ob, int n, const int* a, const int* b, const float* c, const int* sa, const int* sb, float* d, hipStream_t s) {
    if (oa == 0 && ob == 0) return launch<FA, FB, 0, 0>(n, a, b, c, sa, sb, d, s);
    if constexpr (FA == 0 && FB == 0) {
        switch (oa * 4 + ob) {
#define QS_CASE(OA, OB) case OA * 4 + OB: return launch<0, 0, OA, OB>(n, a, b, c, sa, sb, d, s);
            QS_CASE(0, 1) QS_CASE(0, 2) QS_CASE(0, 3) QS_CASE(1, 0) QS_CASE(1, 1) QS_CASE(1, 2) QS_CASE(1, 3) QS_CASE(2, 0) QS_CASE(2, 1)
            QS_CASE(2, 2) QS_CASE(2, 3) QS_CASE(3, 0) QS_CASE(3, 1) QS_CASE(3, 2) QS_CASE(3, 3)
#undef QS_CASE
        }
    }
    return -1;          // opsel other than 0 is probed with FP8 E4M3 on both sides only
}

template <int FA>
static int by_fb(int fb, int oa, int ob, int n, const int* a, const int* b, const float* c, const int* sa, const int* sb, float* d, hipStream_t s) {
    switch (fb) {
        case 0: return by_opsel<FA, 0>(oa, ob, n, a, b, c, sa, sb, d, s);
        case 1: return by_opsel<FA, 1>(oa, ob, n, a, b, c, sa, sb, d, s);
        case 2: return by_opsel<FA, 2>(oa, ob, n, a, b, c, sa, sb, d, s);
        case 3: return by_opsel<FA, 3>(oa, ob, n, a, b, c, sa, sb, d, s);
        case 4: return by_opsel<FA, 4>(oa, ob, n, a, b, c, sa, sb, d, s);
    }
    return -1;
}

extern "C" int probe_mfma_scale(int fa, int fb, int oa, int ob, int n, const int* a, const int* b, const float* c, const int* sa,
                                const int* sb, float* d, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    switch (fa) {
        case 0: return by_fb<0>(fb, oa, ob, n, a, b, c, sa, sb, d, s);
        case 1: return by_fb<1>(fb, oa, ob, n, a, b, c, sa, sb, d, s);
        case 2: return by_fb<2>(fb, oa, ob, n, a, b, c, sa, sb, d, s);
        case 3: return by_fb<3>(fb, oa, ob, n, a, b, c, sa, sb, d, s);
        case 4: return by_fb<4>(fb, oa, ob, n, a, b, c, sa, sb, d, s);
    }
    return -1;
}
