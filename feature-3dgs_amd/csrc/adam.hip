// adam.hip - one Adam step over one parameter tensor (optimizer part).
//
// Semantics: torch.optim.Adam as the reference configures it (scene/gaussian_model.py:163-178: eps = 1e-15, default
// betas, no weight decay, no amsgrad), i.e. per element
//     m = m + (1 - b1)(g - m);  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The reference steps seven tensors with torch's multi-kernel foreach path; this is ONE streaming pass per tensor:
// 16 bytes read + 12 written per element, float4-vectorised.
//
// The capturable form (include/f3dgs.h: f3dgs_adam_schedule + f3dgs_adam_step_multi_device) keeps t, lr and the two
// bias-correction constants on the device: one wave advances the step words and forms the constants, the step kernel reads
// them - so a launch replayed from a graph takes the step it runs in.  Also here: the in-place opacity reset.
#include "common.h"

namespace f3dgs {

namespace {

// One element's update; every loop below goes through it, so the vector path, the ragged tail and the masked
// variant round identically (explicit fmaf: no contraction choices left to the compiler).
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float step_size, float b2, float omb1,
                                            float omb2, float inv_sqrt_bc2, float eps) {
    m = fmaf(omb1, g - m, m);                  // torch: exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(b2, v, (omb2 * g) * g);
    p -= step_size * (m / fmaf(sqrtf(v), inv_sqrt_bc2, eps));
}

__global__ void __launch_bounds__(256)
adam_kernel(size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
            float step_size, float b1, float b2, float omb1, float omb2, float inv_sqrt_bc2, float eps,
            const uint8_t* __restrict__ row_mask, uint32_t width) {
    const size_t i4 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (row_mask) {
        // visibility-masked variant: rows whose mask byte is 0 keep parameter AND moments (no decay) - they cost one
        // byte of traffic instead of 28 per element
        const size_t last = (i4 + 4 <= n ? i4 + 4 : n) - 1;
        const size_t r0 = i4 / width, r1 = last / width;
        bool any = false;
        for (size_t r = r0; r <= r1; r++) any = any || row_mask[r] != 0;
        if (!any) return;
        for (size_t i = i4; i <= last; i++) {
            if (!row_mask[i / width]) continue;
            adam_update(p[i], g[i], m[i], v[i], step_size, b2, omb1, omb2, inv_sqrt_bc2, eps);
        }
        return;
    }
    if (i4 + 4 <= n && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                         reinterpret_cast<uintptr_t>(v)) & 15) == 0) {
        float4 pp = *reinterpret_cast<float4*>(p + i4), mm = *reinterpret_cast<float4*>(m + i4), vv = *reinterpret_cast<float4*>(v + i4);
        const float4 gg = *reinterpret_cast<const float4*>(g + i4);
        float* pa = &pp.x; float* ma = &mm.x; float* va = &vv.x; const float* ga = &gg.x;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            adam_update(pa[k], ga[k], ma[k], va[k], step_size, b2, omb1, omb2, inv_sqrt_bc2, eps);
        }
        *reinterpret_cast<float4*>(p + i4) = pp;
        *reinterpret_cast<float4*>(m + i4) = mm;
        *reinterpret_cast<float4*>(v + i4) = vv;
        return;
    }
    for (size_t i = i4; i < n && i < i4 + 4; i++) {
        adam_update(p[i], g[i], m[i], v[i], step_size, b2, omb1, omb2, inv_sqrt_bc2, eps);
    }
}

// ---- several tensors, one launch: block b belongs to the tensor whose block range contains it ------------------------------
struct AdamEntry {
    float* p; const float* g; float* m; float* v;
    size_t n;
    uint32_t block0;         // first workgroup of this tensor
    uint32_t width;          // floats per row (row mask variant), 0: the mask does not apply to this tensor
    float step_size, inv_sqrt_bc2;
};
struct AdamTable {
    AdamEntry t[F3DGS_ADAM_MAX_TENSORS];
    int count;
};

// One workgroup's share of one table entry: the float4 path, the ragged tail and the row-mask variant.  Both multi-tensor
// kernels below go through it and differ only in where the entry's two constants come from.
__device__ __forceinline__ void adam_entry_block(const AdamEntry& e, float step_size, float inv_sqrt_bc2, float b2, float omb1,
                                                 float omb2, float eps, const uint8_t* __restrict__ row_mask) {
    const size_t i4 = ((size_t)(blockIdx.x - e.block0) * 256 + threadIdx.x) * 4;
    if (i4 >= e.n) return;
    float* __restrict__ p = e.p; const float* __restrict__ g = e.g; float* __restrict__ m = e.m; float* __restrict__ v = e.v;
    if (row_mask && e.width) {
        const size_t last = (i4 + 4 <= e.n ? i4 + 4 : e.n) - 1;
        const size_t r0 = i4 / e.width, r1 = last / e.width;
        bool any = false;
        for (size_t r = r0; r <= r1; r++) any = any || row_mask[r] != 0;
        if (!any) return;
        for (size_t i = i4; i <= last; i++) {
            if (!row_mask[i / e.width]) continue;
            adam_update(p[i], g[i], m[i], v[i], step_size, b2, omb1, omb2, inv_sqrt_bc2, eps);
        }
        return;
    }
    if (i4 + 4 <= e.n && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                           reinterpret_cast<uintptr_t>(v)) & 15) == 0) {
        float4 pp = *reinterpret_cast<float4*>(p + i4), mm = *reinterpret_cast<float4*>(m + i4), vv = *reinterpret_cast<float4*>(v + i4);
        const float4 gg = *reinterpret_cast<const float4*>(g + i4);
        float* pa = &pp.x; float* ma = &mm.x; float* va = &vv.x; const float* ga = &gg.x;
#pragma unroll
        for (int q = 0; q < 4; q++) adam_update(pa[q], ga[q], ma[q], va[q], step_size, b2, omb1, omb2, inv_sqrt_bc2, eps);
        *reinterpret_cast<float4*>(p + i4) = pp;
        *reinterpret_cast<float4*>(m + i4) = mm;
        *reinterpret_cast<float4*>(v + i4) = vv;
        return;
    }
    for (size_t i = i4; i < e.n && i < i4 + 4; i++) adam_update(p[i], g[i], m[i], v[i], step_size, b2, omb1, omb2, inv_sqrt_bc2, eps);
}

// DEVICE_CONSTS = false: the constants the host formed, from the entry (f3dgs_adam_step_multi).  true: from consts[k], which
// adam_schedule_kernel wrote earlier on the stream (f3dgs_adam_step_multi_device); k is the same for the whole workgroup, so
// that read is a uniform (scalar) load.
template <bool DEVICE_CONSTS>
__device__ __forceinline__ void adam_multi_body(const AdamTable& tab, const f3dgs_adam_consts* __restrict__ consts, float b2,
                                                float omb1, float omb2, float eps, const uint8_t* __restrict__ row_mask) {
    int k = 0;
#pragma unroll 1
    while (k + 1 < tab.count && blockIdx.x >= tab.t[k + 1].block0) k++;
    const AdamEntry e = tab.t[k];
    float step_size = e.step_size, inv_sqrt_bc2 = e.inv_sqrt_bc2;
    if (DEVICE_CONSTS) {
        const f3dgs_adam_consts c = consts[k];
        step_size = c.step_size;
        inv_sqrt_bc2 = c.inv_sqrt_bc2;
    }
    adam_entry_block(e, step_size, inv_sqrt_bc2, b2, omb1, omb2, eps, row_mask);
}

__global__ void __launch_bounds__(256)
adam_multi_kernel(AdamTable tab, float b2, float omb1, float omb2, float eps, const uint8_t* __restrict__ row_mask) {
    adam_multi_body<false>(tab, nullptr, b2, omb1, omb2, eps, row_mask);
}

__global__ void __launch_bounds__(256)
adam_multi_device_kernel(AdamTable tab, const f3dgs_adam_consts* __restrict__ consts, float b2, float omb1, float omb2, float eps,
                         const uint8_t* __restrict__ row_mask) {
    adam_multi_body<true>(tab, consts, b2, omb1, omb2, eps, row_mask);
}

// ---- step counts, rates and the two constants on the device ---------------------------------------------------------------
// The rate of a scheduled tensor at iteration i, in fp64: log-linear from lr_init (i = 0) to lr_final (i >= max_steps), both
// zero meaning "frozen"; scaled during the first lr_delay_steps iterations by a factor that rises from lr_delay_mult to 1
// along a quarter sine wave.
__device__ __forceinline__ double scheduled_rate(const f3dgs_adam_device_tensor& t, double i) {
    if (t.lr_init == 0.0 && t.lr_final == 0.0) return 0.0;
    double delay = 1.0;
    if (t.lr_delay_steps > 0) {
        const double w = fmin(fmax(i / (double)t.lr_delay_steps, 0.0), 1.0);
        delay = t.lr_delay_mult + (1.0 - t.lr_delay_mult) * sin(1.5707963267948966 * w);
    }
    const double u = fmin(fmax(i / (double)t.max_steps, 0.0), 1.0);
    return delay * exp(log(t.lr_init) * (1.0 - u) + log(t.lr_final) * u);
}

struct AdamScheduleTable {
    f3dgs_adam_device_tensor t[F3DGS_ADAM_MAX_TENSORS];
    int count;
};

// One wave; lane k serves table entry k.  Every lane reads the iteration word before lane 0 stores the advanced one (the
// barrier keeps that order whatever the compiler does with the loads).
__global__ void __launch_bounds__(64)
adam_schedule_kernel(AdamScheduleTable tab, double b1, double b2, long long* __restrict__ iteration, int advance,
                     f3dgs_adam_consts* __restrict__ consts) {
    const int k = threadIdx.x;
    long long it = 0;
    if (iteration) it = *iteration + (advance ? 1 : 0);
    __syncthreads();
    if (k == 0 && iteration && advance) *iteration = it;
    if (k >= tab.count) return;
    const f3dgs_adam_device_tensor& e = tab.t[k];
    if (e.n == 0) return;
    const float t = *e.step + 1.0f;
    *e.step = t;
    const double lr = e.scheduled ? scheduled_rate(e, (double)it) : *e.lr;
    // formed in double and rounded once, as launch_adam_step_multi does on the host
    const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    f3dgs_adam_consts c;
    c.lr_now = lr;
    c.step_size = (float)(lr / bc1);
    c.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    consts[k] = c;
}

// ---- the reference's reset_opacity without a new Parameter -----------------------------------------------------------------
__global__ void __launch_bounds__(256)
reset_opacity_kernel(size_t n, float* __restrict__ raw, float* __restrict__ m, float* __restrict__ v, float cap) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float s = 1.0f / (1.0f + expf(-raw[i]));          // model_front.hip's sigmoid
    const float x = fminf(s, cap);                          // torch.min: a NaN stays a NaN
    raw[i] = (s != s) ? s : logf(x / (1.0f - x));           // inverse_sigmoid
    if (m) m[i] = 0.0f;
    if (v) v[i] = 0.0f;
}

void launch_adam_step_multi(int count, const f3dgs_adam_tensor* tensors, double b1, double b2, double eps, const uint8_t* row_mask,
                            size_t rows, hipStream_t s) {
    AdamTable tab;
    tab.count = 0;
    uint32_t blocks = 0;
    for (int i = 0; i < count; i++) {
        const f3dgs_adam_tensor& t = tensors[i];
        if (t.n == 0) continue;
        AdamEntry& e = tab.t[tab.count++];
        e.p = t.param; e.g = t.grad; e.m = t.exp_avg; e.v = t.exp_avg_sq; e.n = t.n;
        e.block0 = blocks;
        e.width = (row_mask && rows && t.n % rows == 0) ? (uint32_t)(t.n / rows) : 0u;
        // every derived constant is formed in double and rounded once, as in launch_adam_step
        const double bc1 = 1.0 - pow(b1, (double)t.step), bc2 = 1.0 - pow(b2, (double)t.step);
        e.step_size = (float)(t.lr / bc1);
        e.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        blocks += (uint32_t)(((t.n + 3) / 4 + 255) / 256);
    }
    if (tab.count == 0) return;
    hipLaunchKernelGGL(adam_multi_kernel, dim3(blocks), dim3(256), 0, s, tab, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2),
                       (float)eps, row_mask);
}

void launch_adam_schedule(int count, const f3dgs_adam_device_tensor* tensors, double b1, double b2, long long* iteration, int advance,
                          f3dgs_adam_consts* consts, hipStream_t s) {
    AdamScheduleTable tab;
    tab.count = count;
    bool any = false;
    for (int i = 0; i < count; i++) {
        tab.t[i] = tensors[i];
        any = any || tensors[i].n != 0;
    }
    if (!any) return;        // nothing is stepped: no step word moves, and neither does the iteration
    hipLaunchKernelGGL(adam_schedule_kernel, dim3(1), dim3(64), 0, s, tab, b1, b2, iteration, advance, consts);
}

void launch_adam_step_multi_device(int count, const f3dgs_adam_device_tensor* tensors, double b1, double b2, double eps,
                                   const uint8_t* row_mask, size_t rows, const f3dgs_adam_consts* consts, hipStream_t s) {
    // entry k stays entry k (consts[k] is its slot): an empty tensor keeps its place with no workgroups of its own
    AdamTable tab;
    tab.count = count;
    uint32_t blocks = 0;
    for (int i = 0; i < count; i++) {
        const f3dgs_adam_device_tensor& t = tensors[i];
        AdamEntry& e = tab.t[i];
        e.p = t.param; e.g = t.grad; e.m = t.exp_avg; e.v = t.exp_avg_sq; e.n = t.n;
        e.block0 = blocks;
        e.width = (row_mask && rows && t.n && t.n % rows == 0) ? (uint32_t)(t.n / rows) : 0u;
        e.step_size = 0.f;
        e.inv_sqrt_bc2 = 0.f;
        blocks += (uint32_t)(((t.n + 3) / 4 + 255) / 256);
    }
    if (blocks == 0) return;
    hipLaunchKernelGGL(adam_multi_device_kernel, dim3(blocks), dim3(256), 0, s, tab, consts, (float)b2, (float)(1.0 - b1),
                       (float)(1.0 - b2), (float)eps, row_mask);
}

void launch_reset_opacity(size_t n, float* raw, float* exp_avg, float* exp_avg_sq, float cap, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(reset_opacity_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, n, raw, exp_avg, exp_avg_sq, cap);
}

void launch_adam_step(size_t n, float* p, const float* g, float* m, float* v, double lr, double b1, double b2, double eps, int step,
                      const uint8_t* row_mask, size_t width, hipStream_t s) {
    if (n == 0) return;
    // every derived constant is formed in double from the caller's doubles and rounded once, like torch does
    // (1 - 0.999f in float is off by 1.3e-5 relative)
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    const size_t threads = (n + 3) / 4;
    hipLaunchKernelGGL(adam_kernel, dim3((threads + 255) / 256), dim3(256), 0, s, n, p, g, m, v, (float)(lr / bc1), (float)b1,
                       (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)(1.0 / sqrt(bc2)), (float)eps, row_mask, (uint32_t)(width ? width : 1));
}

// The checks f3dgs_adam_schedule and f3dgs_adam_step_multi_device share: both take the same table.
int check_adam_device_table(const char* who, int n_tensors, const f3dgs_adam_device_tensor* tensors, double beta1, double beta2,
                            const void* consts, size_t* blocks_out) {
    if (n_tensors < 0 || n_tensors > F3DGS_ADAM_MAX_TENSORS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: 0 .. %d tensors per call", who, F3DGS_ADAM_MAX_TENSORS);
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: betas (%g, %g) outside [0, 1)", who, beta1, beta2);
    *blocks_out = 0;
    if (n_tensors == 0) return F3DGS_OK;
    if (!tensors) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null table", who);
    if (!consts) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null table of constants", who);
    if (reinterpret_cast<uintptr_t>(consts) & 7) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: the table of constants must be 8-byte aligned", who);
    size_t blocks = 0;
    for (int i = 0; i < n_tensors; i++) {
        const f3dgs_adam_device_tensor& t = tensors[i];
        if (t.scheduled) {
            if (t.max_steps <= 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: tensor %d: max_steps = %lld", who, i, t.max_steps);
            if (t.lr_delay_steps < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: tensor %d: lr_delay_steps = %lld", who, i, t.lr_delay_steps);
            if (!(t.lr_init >= 0.0) || !(t.lr_final >= 0.0) || ((t.lr_init == 0.0) != (t.lr_final == 0.0)))
                return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: tensor %d: rates %g -> %g: both positive or both zero", who, i, t.lr_init, t.lr_final);
        }
        if (t.n == 0) continue;
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: tensor %d: null pointer", who, i);
        if (!t.step) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: tensor %d: null step word", who, i);
        if (!t.scheduled && !t.lr) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: tensor %d: null rate word", who, i);
        blocks += ((t.n + 3) / 4 + 255) / 256;
    }
    if (blocks >= (1ull << 31)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: too large for one launch", who);
    *blocks_out = blocks;
    return F3DGS_OK;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

int f3dgs_adam_step(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                    double beta2, double eps, int step, void* stream) {
    return f3dgs_adam_step_rows(n, 1, nullptr, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, stream);
}

int f3dgs_adam_step_rows(size_t n, size_t width, const uint8_t* row_mask, float* param, const float* grad, float* exp_avg,
                         float* exp_avg_sq, double lr, double beta1, double beta2, double eps, int step, void* stream) {
    if (n == 0) return F3DGS_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "null pointer");
    if (step < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "step counts from 1");
    if (row_mask && (width == 0 || n % width != 0 || width > 0xFFFFFFFFull))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "n = %zu is not a whole number of rows of %zu floats", n, width);
    launch_adam_step(n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, row_mask, width, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return F3DGS_OK;
}

int f3dgs_adam_step_multi(int n_tensors, const f3dgs_adam_tensor* tensors, double beta1, double beta2, double eps,
                          const uint8_t* row_mask, size_t rows, void* stream) {
    if (n_tensors < 0 || n_tensors > F3DGS_ADAM_MAX_TENSORS) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "0 .. %d tensors per call", F3DGS_ADAM_MAX_TENSORS);
    if (n_tensors == 0) return F3DGS_OK;
    if (!tensors) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "null table");
    size_t blocks = 0;
    for (int i = 0; i < n_tensors; i++) {
        const f3dgs_adam_tensor& t = tensors[i];
        if (t.n == 0) continue;
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "tensor %d: null pointer", i);
        if (t.step < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "tensor %d: step counts from 1", i);
        blocks += ((t.n + 3) / 4 + 255) / 256;
    }
    if (blocks >= (1ull << 31)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "too large for one launch");
    if (row_mask && rows == 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "row mask without a row count");
    launch_adam_step_multi(n_tensors, tensors, beta1, beta2, eps, row_mask, rows, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return F3DGS_OK;
}

int f3dgs_adam_schedule(int n_tensors, const f3dgs_adam_device_tensor* tensors, double beta1, double beta2, long long* iteration,
                        int advance, f3dgs_adam_consts* consts, void* stream) {
    size_t blocks = 0;
    if (int rc = check_adam_device_table("f3dgs_adam_schedule", n_tensors, tensors, beta1, beta2, consts, &blocks)) return rc;
    if (n_tensors == 0) return F3DGS_OK;
    for (int i = 0; i < n_tensors; i++)
        if (tensors[i].scheduled && !iteration)
            return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "f3dgs_adam_schedule: tensor %d is scheduled, but there is no iteration word", i);
    if (reinterpret_cast<uintptr_t>(iteration) & 7) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "f3dgs_adam_schedule: misaligned iteration word");
    launch_adam_schedule(n_tensors, tensors, beta1, beta2, iteration, advance, consts, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return F3DGS_OK;
}

int f3dgs_adam_step_multi_device(int n_tensors, const f3dgs_adam_device_tensor* tensors, double beta1, double beta2, double eps,
                                 const uint8_t* row_mask, size_t rows, const f3dgs_adam_consts* consts, void* stream) {
    size_t blocks = 0;
    if (int rc = check_adam_device_table("f3dgs_adam_step_multi_device", n_tensors, tensors, beta1, beta2, consts, &blocks)) return rc;
    if (row_mask && rows == 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "f3dgs_adam_step_multi_device: row mask without a row count");
    if (n_tensors == 0) return F3DGS_OK;
    launch_adam_step_multi_device(n_tensors, tensors, beta1, beta2, eps, row_mask, rows, consts, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return F3DGS_OK;
}

int f3dgs_reset_opacity(size_t n, float* raw, float* exp_avg, float* exp_avg_sq, float cap, void* stream) {
    if (!(cap > 0.f && cap < 1.f)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "f3dgs_reset_opacity: cap = %g outside (0, 1)", (double)cap);
    if (n == 0) return F3DGS_OK;
    if (!raw) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "f3dgs_reset_opacity: null pointer");
    if (n >= (1ull << 39)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "f3dgs_reset_opacity: too large for one launch");
    launch_reset_opacity(n, raw, exp_avg, exp_avg_sq, cap, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return F3DGS_OK;
}

}  // extern "C"
