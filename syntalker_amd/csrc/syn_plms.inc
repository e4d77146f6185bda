// Pseudo linear multistep sampling (diffusion/gaussian_diffusion.py:1004-1086): the history of noise estimates, kept on the device.
//
// A PLMS step is a syn_denoise_step whose coefficient row carries the Adams-Bashforth weight of the step's own estimate and whose `noise`
// operand is H, the weighted sum of the earlier estimates (DESIGN.md, "PLMS").  This kernel runs after the step: from the x_t the step read
// and the x0_hat it wrote it forms e_new = (r x_t - x0_hat) / m, stores it over the oldest slot of a ring of three, and writes the H of the
// NEXT step.  Everything is per element and x_t, x0_hat, the ring and H share one element order, so token-major and fragment-order latents
// take the same kernel.  The row of the table (r, 1 / m, the next step's weights by ring slot, the slot to overwrite) is picked by the
// device-side step counter that k_step_advance maintains: a captured graph replays for every step.
namespace {
namespace plms {

// per element: reads x_t and x0_hat (8 B) and up to two ring slots (8 B), writes a ring slot (4 B, when the estimate is read again) and H (4 B):
// 12 B at order 2, 20 at order 3, 24 at order 4
__global__ __launch_bounds__(256) void k_plms_update(const syn_plms_row* __restrict__ table, int n_rows, const int* __restrict__ counter, int back,
                                                    const f32x4* __restrict__ xt, const f32x4* __restrict__ x0, f32x4* __restrict__ ring,
                                                    f32x4* __restrict__ H, long n4) {
    const int idx = *counter - back;
    if (idx < 0 || idx >= n_rows) return;                 // a counter outside the table: nothing is read or written
    const syn_plms_row row = table[idx];
    const int store = row.store;
    const bool own = store >= 0 || row.w_new != 0.f;      // the step's own estimate is needed
    const bool any = own || row.h_x != 0.f || row.w[0] != 0.f || row.w[1] != 0.f || row.w[2] != 0.f;
    if (!any || store > 2) return;                        // (the steps nothing follows: H is not read again)
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 x = {0.f, 0.f, 0.f, 0.f}, e = x, acc = x;
        if (own || row.h_x != 0.f) x = xt[i];
        if (own) {
            const f32x4 p = x0[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                e[c] = __builtin_fmaf(row.r, x[c], -p[c]) * row.inv_m;
                acc[c] = row.w_new * e[c];
            }
        }
        if (row.h_x != 0.f) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_fmaf(row.h_x, x[c], acc[c]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (row.w[k] != 0.f && k != store) {          // (the slot being overwritten holds the estimate that leaves the history)
                const f32x4 o = ring[(long)k * n4 + i];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = __builtin_fmaf(row.w[k], o[c], acc[c]);
            }
        }
        if (store >= 0) ring[(long)store * n4 + i] = e;
        H[i] = acc;
    }
}

}  // namespace plms
}  // namespace

extern "C" int syn_plms_update(const syn_plms_row* table, int32_t n_rows, const int32_t* counter, int32_t back, const float* x_t, const float* pred_x0,
                               float* ring, float* h, int64_t n, void* stream) {
    if (!table || n_rows <= 0 || !counter || back < 0 || !x_t || !pred_x0 || !ring || !h || n <= 0 || n % 4)
        return fail_msg("syn_plms_update: null pointer, empty table, negative `back`, or n not a positive multiple of 4");
    if (((uintptr_t)x_t | (uintptr_t)pred_x0 | (uintptr_t)ring | (uintptr_t)h) & 15)
        return fail_msg("syn_plms_update: x_t, pred_x0, ring and h must be 16-byte aligned");
    const long n4 = (long)(n / 4);
    const long want = (n4 + 255) / 256, cap = (long)device_cus() * 8;       // a grid sized from the CU count, grid-stride over the rest
    hipLaunchKernelGGL(plms::k_plms_update, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, (hipStream_t)stream, table, (int)n_rows,
                       (const int*)counter, (int)back, (const f32x4*)x_t, (const f32x4*)pred_x0, (f32x4*)ring, (f32x4*)h, n4);
    return launched("k_plms_update launch");
}
