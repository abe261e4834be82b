// binding.cpp — pybind11 / libtorch front-end `diff_gaussian_rasterization._C`.
//
// Reproduces the three Python-visible entry points of the reference binding
//   rasterize_gaussians            (reference: rasterize_points.cu:35-124,  ext.cpp:16)
//   rasterize_gaussians_backward   (reference: rasterize_points.cu:126-215, ext.cpp:17)
//   mark_visible                   (reference: rasterize_points.cu:217-236, ext.cpp:18)
// with identical positional signatures and return tuples, on top of the C ABI of
// libf3dgs_hip.so (include/f3dgs.h).  PyTorch is plumbing only: tensor allocation through the
// caching allocator, the current HIP stream, and the three growable byte buffers.
//
// Differences to the reference binding, all deliberate:
//   * the feature dimension C is read from semantic_feature.size(-1) instead of a compile-time macro;
//   * work is enqueued on PyTorch's CURRENT stream (the reference uses the legacy default stream);
//   * outputs / gradients are torch::empty (the kernels overwrite every element) — no zero-fill passes;
//   * inputs that are not on a HIP device raise instead of silently reading host memory.

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <array>
#include <exception>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/f3dgs.h"

namespace py = pybind11;

namespace {

const float* fptr(const torch::Tensor& t) { return t.numel() ? t.data_ptr<float>() : nullptr; }

char* resize_hook(void* ctx, size_t n) {
    auto* t = static_cast<torch::Tensor*>(ctx);
    t->resize_({(long long)n});
    return reinterpret_cast<char*>(t->data_ptr());
}

void check_status(int rc, const char* where) {
    if (rc != F3DGS_OK) throw std::runtime_error(std::string(where) + ": " + f3dgs_last_error());
}

torch::Tensor dev_f32(const torch::Tensor& t, const char* name) {
    if (t.numel() == 0) return t;
    TORCH_CHECK(t.is_cuda(), name, " must live on a HIP device (got ", t.device(), "): the MI355X rasterizer has no CPU path");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32");
    torch::Tensor c = t.contiguous();
    // the library reads rows with 16-byte accesses (f3dgs.h, Alignment): a view at an odd storage offset is copied into a fresh
    // (allocator-aligned) tensor instead of being refused - the reference accepts such views
    if (reinterpret_cast<uintptr_t>(c.data_ptr()) & 15) c = c.clone();
    return c;
}

// The kernels index the feature tensor as (P, C): the reference's layout is (P, 1, C) (scene/gaussian_model.py:
// `_semantic_feature`, rasterize_points.cu:160).  Anything else with more than C floats per Gaussian would be
// read with the wrong stride, so it is rejected instead.
int feature_channels(const torch::Tensor& semantic_feature, int64_t P) {
    if (semantic_feature.numel() == 0) return semantic_feature.dim() >= 1 ? (int)semantic_feature.size(-1) : 0;
    TORCH_CHECK(semantic_feature.dim() == 3 && semantic_feature.size(0) == P && semantic_feature.size(1) == 1,
                "semantic_feature must have dimensions (num_points, 1, C); got ", semantic_feature.sizes());
    return (int)semantic_feature.size(2);
}

// Python callable invoked with dL_dsemantic_feature as soon as the blend backward has been enqueued
// (include/f3dgs.h: f3dgs_set_feature_grad_ready_callback).  The GIL is held throughout the binding call.
py::object& feature_grad_hook() {
    static py::object* hook = new py::object(py::none());   // leaked on purpose: no destructor after interpreter exit
    return *hook;
}
// A Python exception must not unwind through the extern "C" frame of f3dgs_backward: it is parked here and rethrown by the
// binding once the C call has returned and the callback registration has been cleared.
std::exception_ptr& pending_hook_error() {
    thread_local std::exception_ptr e;
    return e;
}
void feature_ready_trampoline(void* ctx, void* /*stream*/) {
    py::object& hook = feature_grad_hook();
    if (hook.is_none() || pending_hook_error()) return;
    try {
        hook(*static_cast<torch::Tensor*>(ctx));
    } catch (...) {
        pending_hook_error() = std::current_exception();
    }
}
// clears the thread-local callback registration on every way out of the backward binding
struct FeatureCallbackGuard {
    bool armed;
    explicit FeatureCallbackGuard(bool on, void* ctx) : armed(on) {
        if (armed) f3dgs_set_feature_grad_ready_callback(feature_ready_trampoline, ctx);
    }
    ~FeatureCallbackGuard() {
        if (armed) f3dgs_set_feature_grad_ready_callback(nullptr, nullptr);
    }
};

// Accumulation buffer for the feature gradient across the views of one optimiser step (include/f3dgs.h:
// f3dgs_set_feature_grad_accumulate): while it is set, the backward binding hands IT to the library as
// dL_dsemantic_feature (accumulate mode) and returns an empty tensor in its place - the Python side then reports "no
// gradient" for the input to autograd, the sum lives in the buffer (normally the leaf's .grad).
torch::Tensor& feature_grad_accumulator() {
    static torch::Tensor* t = new torch::Tensor();
    return *t;
}
// set_feature_grad_lowres: (gx (Hg,Wg,C), scale (0-dim) or undefined), consumed by the next backward call
std::pair<torch::Tensor, torch::Tensor>& feature_grad_lowres() {
    static std::pair<torch::Tensor, torch::Tensor> t;
    return t;
}

struct AccumulateGuard {
    bool armed;
    explicit AccumulateGuard(bool on) : armed(on) { if (armed) f3dgs_set_feature_grad_accumulate(1); }
    ~AccumulateGuard() { if (armed) f3dgs_set_feature_grad_accumulate(0); }
};

// Python callable invoked as fn(row_begin, row_end, {"sh": dL_dsh, "means3D": ..., ...}) after every row chunk of the
// per-Gaussian stage has been enqueued (include/f3dgs.h: f3dgs_set_grad_rows_ready_callback), and its chunk count.
py::object& grad_rows_hook() {
    static py::object* hook = new py::object(py::none());
    return *hook;
}
int& grad_rows_chunks() {
    static int chunks = 1;
    return chunks;
}
struct RowsCallbackCtx {
    const torch::Tensor *sh, *means3D, *scales, *rotations, *opacities, *colors, *means2D, *cov3D;
};
void rows_ready_trampoline(void* ctx, void* /*stream*/, int row_begin, int row_end) {
    py::object& hook = grad_rows_hook();
    if (hook.is_none() || pending_hook_error()) return;
    try {
        const auto* c = static_cast<const RowsCallbackCtx*>(ctx);
        py::dict grads;
        grads["sh"] = *c->sh; grads["means3D"] = *c->means3D; grads["scales"] = *c->scales; grads["rotations"] = *c->rotations;
        grads["opacities"] = *c->opacities; grads["colors_precomp"] = *c->colors; grads["means2D"] = *c->means2D;
        grads["cov3Ds_precomp"] = *c->cov3D;
        hook(row_begin, row_end, grads);
    } catch (...) {
        pending_hook_error() = std::current_exception();
    }
}
struct RowsCallbackGuard {
    bool armed;
    RowsCallbackGuard(bool on, void* ctx, int chunks) : armed(on) {
        if (armed) f3dgs_set_grad_rows_ready_callback(rows_ready_trampoline, ctx, chunks);
    }
    ~RowsCallbackGuard() {
        if (armed) f3dgs_set_grad_rows_ready_callback(nullptr, nullptr, 1);
    }
};

void* current_stream(const torch::Tensor& ref) {
    return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(ref.device().index()).stream();
}

std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussians(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors,
                   const torch::Tensor& semantic_feature, const torch::Tensor& opacity, const torch::Tensor& scales,
                   const torch::Tensor& rotations, const float scale_modifier, const torch::Tensor& cov3D_precomp,
                   const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, const float tan_fovx,
                   const float tan_fovy, const int image_height, const int image_width, const torch::Tensor& sh,
                   const int degree, const torch::Tensor& campos, const bool prefiltered, const bool debug) {
    if (means3D.ndimension() != 2 || means3D.size(1) != 3) {
        AT_ERROR("means3D must have dimensions (num_points, 3)");  // rasterize_points.cu:58-60
    }
    TORCH_CHECK(means3D.is_cuda(), "means3D must live on a HIP device: the MI355X rasterizer has no CPU path");
    const int P = means3D.size(0);
    const int H = image_height, W = image_width;
    const int C = feature_channels(semantic_feature, P);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());

    auto f32 = means3D.options().dtype(torch::kFloat32);
    torch::Tensor out_color = torch::empty({3, H, W}, f32);
    torch::Tensor out_depth = torch::empty({1, H, W}, f32);
    torch::Tensor out_feature_map = torch::empty({C, H, W}, f32);
    torch::Tensor radii = torch::empty({P}, means3D.options().dtype(torch::kInt32));
    auto u8 = means3D.options().dtype(torch::kByte);
    torch::Tensor geomBuffer = torch::empty({0}, u8);
    torch::Tensor binningBuffer = torch::empty({0}, u8);
    torch::Tensor imgBuffer = torch::empty({0}, u8);

    auto bg = dev_f32(background, "bg"), m3 = dev_f32(means3D, "means3D"), col = dev_f32(colors, "colors_precomp"),
         sf = dev_f32(semantic_feature, "semantic_feature"), op = dev_f32(opacity, "opacities"),
         sc = dev_f32(scales, "scales"), rot = dev_f32(rotations, "rotations"), cov = dev_f32(cov3D_precomp, "cov3D_precomp"),
         vm = dev_f32(viewmatrix, "viewmatrix"), pm = dev_f32(projmatrix, "projmatrix"), shs = dev_f32(sh, "sh"),
         cp = dev_f32(campos, "campos");
    int M = 0;
    if (shs.numel() != 0) M = shs.size(1);

    int rendered = 0;
    const int rc = f3dgs_forward(resize_hook, &geomBuffer, resize_hook, &binningBuffer, resize_hook, &imgBuffer, P, degree,
                                 M, C, fptr(bg), W, H, fptr(m3), fptr(shs), fptr(col), fptr(sf), fptr(op), fptr(sc),
                                 scale_modifier, fptr(rot), fptr(cov), fptr(vm), fptr(pm), fptr(cp), tan_fovx, tan_fovy,
                                 prefiltered ? 1 : 0, out_color.data_ptr<float>(),
                                 C ? out_feature_map.data_ptr<float>() : nullptr, out_depth.data_ptr<float>(),
                                 P ? radii.data_ptr<int>() : nullptr, debug ? 1 : 0, current_stream(means3D), &rendered);
    check_status(rc, "rasterize_gaussians");
    return std::make_tuple(rendered, out_color, out_feature_map, out_depth, radii, geomBuffer, binningBuffer, imgBuffer);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor>
RasterizeGaussiansBackward(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii,
                           const torch::Tensor& colors, const torch::Tensor& semantic_feature,
                           const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier,
                           const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                           const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                           const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_feature,
                           const torch::Tensor& dL_dout_depth, const torch::Tensor& sh, const int degree,
                           const torch::Tensor& campos, const torch::Tensor& geomBuffer, const int R,
                           const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const bool debug) {
    TORCH_CHECK(means3D.is_cuda(), "means3D must live on a HIP device: the MI355X rasterizer has no CPU path");
    const int P = means3D.size(0);
    const int H = dL_dout_color.size(1), W = dL_dout_color.size(2);  // rasterize_points.cu:154-155
    const int C = feature_channels(semantic_feature, P);
    const int F1 = 1;
    c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());

    auto shs = dev_f32(sh, "sh");
    int M = 0;
    if (shs.numel() != 0) M = shs.size(1);

    auto o = means3D.options().dtype(torch::kFloat32);
    torch::Tensor dL_dmeans3D = torch::empty({P, 3}, o);
    torch::Tensor dL_dmeans2D = torch::empty({P, 3}, o);
    torch::Tensor dL_dcolors = torch::empty({P, 3}, o);
    torch::Tensor& acc = feature_grad_accumulator();
    const bool accumulate = acc.defined() && P > 0 && C > 0;
    if (accumulate) {
        TORCH_CHECK(acc.is_cuda() && acc.device() == means3D.device() && acc.scalar_type() == torch::kFloat32 && acc.is_contiguous() &&
                    acc.numel() == (int64_t)P * C,
                    "feature gradient accumulator must be a contiguous float32 tensor of ", P, " x ", C, " elements on the op's device");
    }
    torch::Tensor dL_dsemantic_feature = accumulate ? acc.view({P, F1, C}) : torch::empty({P, F1, C}, o);
    torch::Tensor dL_dopacity = torch::empty({P, 1}, o);
    torch::Tensor dL_dcov3D = torch::empty({P, 6}, o);
    torch::Tensor dL_dsh = torch::empty({P, M, 3}, o);
    torch::Tensor dL_dscales = torch::empty({P, 3}, o);
    torch::Tensor dL_drotations = torch::empty({P, 4}, o);
    auto sc = dev_f32(scales, "scales"), rot = dev_f32(rotations, "rotations");
    if (sc.numel() == 0) {  // cov3D_precomp path: these grads are defined as zero (rasterize_points.cu:171-172)
        dL_dscales.zero_();
        dL_drotations.zero_();
    }
    torch::Tensor scratch = torch::empty({(long long)f3dgs_backward_scratch_bytes(P, C)}, means3D.options().dtype(torch::kByte));

    auto bg = dev_f32(background, "bg"), m3 = dev_f32(means3D, "means3D"), col = dev_f32(colors, "colors_precomp"),
         sf = dev_f32(semantic_feature, "semantic_feature"), cov = dev_f32(cov3D_precomp, "cov3D_precomp"),
         vm = dev_f32(viewmatrix, "viewmatrix"), pm = dev_f32(projmatrix, "projmatrix"), cp = dev_f32(campos, "campos"),
         gc = dev_f32(dL_dout_color, "dL_dout_color"), gd = dev_f32(dL_dout_depth, "dL_dout_depth");
    // The feature-map gradient at the loss's resolution (feature_loss.py, lowres_grad=True): one call only.  What autograd hands
    // over as dL_dout_feature is then the loss's placeholder - a zero-stride expansion of one 0, never materialised - unless
    // another consumer of the feature map contributed a dense gradient, which the kernel adds.
    std::pair<torch::Tensor, torch::Tensor> low;
    std::swap(low, feature_grad_lowres());
    const bool lowres = low.first.defined() && P > 0 && C > 0;
    bool dense_feature_grad = true;
    if (lowres) {
        const auto& gx = low.first;
        TORCH_CHECK(gx.is_cuda() && gx.device() == means3D.device() && gx.scalar_type() == torch::kFloat32 && gx.is_contiguous() &&
                    gx.dim() == 3 && gx.size(2) == C, "low-resolution feature-map gradient must be a contiguous float32 (Hg, Wg, ", C,
                    ") tensor on the op's device");
        TORCH_CHECK(gx.numel() < (1ll << 31), "low-resolution feature-map gradient too large");
        if (low.second.defined())
            TORCH_CHECK(low.second.is_cuda() && low.second.scalar_type() == torch::kFloat32 && low.second.numel() == 1,
                        "the scale of the low-resolution gradient must be a float32 scalar on the device");
        bool all_zero_stride = dL_dout_feature.dim() > 0;
        for (int64_t d = 0; d < dL_dout_feature.dim(); d++) all_zero_stride = all_zero_stride && dL_dout_feature.stride(d) == 0;
        dense_feature_grad = !(dL_dout_feature.numel() == 0 || all_zero_stride);
    }
    auto gf = dense_feature_grad ? dev_f32(dL_dout_feature, "dL_dout_feature") : torch::Tensor();
    auto gfptr = [&]() -> const float* { return dense_feature_grad ? fptr(gf) : nullptr; };
    TORCH_CHECK(radii.is_cuda() || P == 0, "radii must live on a HIP device");
    auto rad = radii.contiguous();

    const bool notify = !feature_grad_hook().is_none() && P > 0 && C > 0;
    pending_hook_error() = nullptr;
    int rc;
    {
    AccumulateGuard guard_acc(accumulate);
    FeatureCallbackGuard guard_cb(notify, &dL_dsemantic_feature);
    RowsCallbackCtx rows_ctx = {&dL_dsh, &dL_dmeans3D, &dL_dscales, &dL_drotations, &dL_dopacity, &dL_dcolors, &dL_dmeans2D, &dL_dcov3D};
    RowsCallbackGuard guard_rows(!grad_rows_hook().is_none() && P > 0, &rows_ctx, grad_rows_chunks());
    if (lowres)
        check_status(f3dgs_set_feature_grad_lowres(low.first.data_ptr<float>(), (int)low.first.size(0), (int)low.first.size(1),
                                                   low.second.defined() ? low.second.data_ptr<float>() : nullptr),
                     "set_feature_grad_lowres");
    rc = f3dgs_backward(
        P, degree, M, C, R, fptr(bg), W, H, fptr(m3), fptr(shs), fptr(col), fptr(sf), fptr(sc), scale_modifier, fptr(rot),
        fptr(cov), fptr(vm), fptr(pm), fptr(cp), tan_fovx, tan_fovy, P ? rad.data_ptr<int>() : nullptr,
        reinterpret_cast<const char*>(geomBuffer.data_ptr()), reinterpret_cast<const char*>(binningBuffer.data_ptr()),
        reinterpret_cast<const char*>(imageBuffer.data_ptr()), fptr(gc), gfptr(), fptr(gd),
        P ? dL_dmeans2D.data_ptr<float>() : nullptr, nullptr, P ? dL_dopacity.data_ptr<float>() : nullptr,
        P ? dL_dcolors.data_ptr<float>() : nullptr, (P && C) ? dL_dsemantic_feature.data_ptr<float>() : nullptr,
        P ? dL_dmeans3D.data_ptr<float>() : nullptr, P ? dL_dcov3D.data_ptr<float>() : nullptr,
        (P && M) ? dL_dsh.data_ptr<float>() : nullptr, P ? dL_dscales.data_ptr<float>() : nullptr,
        P ? dL_drotations.data_ptr<float>() : nullptr, nullptr, P ? scratch.data_ptr() : nullptr, debug ? 1 : 0,
        current_stream(means3D));
    }
    if (pending_hook_error()) {
        std::exception_ptr e = pending_hook_error();
        pending_hook_error() = nullptr;
        std::rethrow_exception(e);
    }
    check_status(rc, "rasterize_gaussians_backward");
    // accumulate mode: the sum lives in the caller's buffer; an empty tensor tells the Python side "no gradient to hand on"
    return std::make_tuple(dL_dmeans2D, dL_dcolors, accumulate ? torch::empty({0}, o) : dL_dsemantic_feature, dL_dopacity, dL_dmeans3D,
                           dL_dcov3D, dL_dsh, dL_dscales, dL_drotations);
}

torch::Tensor markVisible(torch::Tensor& means3D, torch::Tensor& viewmatrix, torch::Tensor& projmatrix) {
    TORCH_CHECK(means3D.is_cuda(), "means3D must live on a HIP device: the MI355X rasterizer has no CPU path");
    const int P = means3D.size(0);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(means3D.device());
    torch::Tensor present = torch::empty({P}, means3D.options().dtype(at::kBool));
    if (P != 0) {
        auto m3 = dev_f32(means3D, "means3D"), vm = dev_f32(viewmatrix, "viewmatrix"), pm = dev_f32(projmatrix, "projmatrix");
        const int rc = f3dgs_mark_visible(P, fptr(m3), fptr(vm), fptr(pm), reinterpret_cast<uint8_t*>(present.data_ptr<bool>()),
                                          current_stream(means3D));
        check_status(rc, "mark_visible");
    }
    return present;
}

// fused resize -> 1x1 decoder -> L1 (include/f3dgs.h: f3dgs_feature_l1); returns (loss, d_feature_map, d_weight, d_bias, gx).
// dense = false: d_feature_map is not produced (empty); gx = dL/d(resized map), (Hg, Wg, C), a view of the call's scratch,
// is what set_feature_grad_lowres hands to the rasterizer's backward.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
FeatureL1(const torch::Tensor& feature_map, const torch::Tensor& gt, const torch::Tensor& weight, const torch::Tensor& bias, bool dense) {
    TORCH_CHECK(feature_map.is_cuda() && gt.is_cuda(), "feature_l1: tensors must live on a HIP device (no CPU path)");
    TORCH_CHECK(feature_map.dim() == 3 && gt.dim() == 3, "feature_l1: feature_map (C,H,W) and gt (Cout,Hg,Wg) expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(feature_map.device());
    auto fm = dev_f32(feature_map, "feature_map"), g = dev_f32(gt, "gt_feature_map");
    const bool dec = weight.numel() > 0;
    torch::Tensor w = weight, b = bias;
    if (dec) {
        w = dev_f32(weight, "weight");
        b = dev_f32(bias, "bias");
        TORCH_CHECK(w.dim() == 2 && w.size(1) == fm.size(0) && w.size(0) == g.size(0) && b.numel() == g.size(0),
                    "feature_l1: weight (Cout,C) / bias (Cout) do not match feature_map / gt");
    }
    const int C = fm.size(0), H = fm.size(1), W = fm.size(2), Cout = g.size(0), Hg = g.size(1), Wg = g.size(2);
    auto o = fm.options();
    torch::Tensor loss = torch::empty({}, o), d_fm = dense ? torch::empty_like(fm) : torch::empty({0}, o);
    torch::Tensor d_w = dec ? torch::empty_like(w) : torch::empty({0}, o), d_b = dec ? torch::empty_like(b) : torch::empty({0}, o);
    torch::Tensor scratch = torch::empty({(long long)f3dgs_feature_l1_scratch_bytes(C, Cout, Hg, Wg, dec ? 1 : 0)},
                                         o.dtype(torch::kByte));
    const int rc = f3dgs_feature_l1(C, H, W, Cout, Hg, Wg, fm.data_ptr<float>(), dec ? w.data_ptr<float>() : nullptr,
                                    dec ? b.data_ptr<float>() : nullptr, g.data_ptr<float>(), loss.data_ptr<float>(),
                                    dense ? d_fm.data_ptr<float>() : nullptr, dec ? d_w.data_ptr<float>() : nullptr,
                                    dec ? d_b.data_ptr<float>() : nullptr, scratch.data_ptr(), current_stream(fm));
    check_status(rc, "feature_l1");
    const float* gxp = f3dgs_feature_l1_lowres_grad(C, Cout, Hg, Wg, dec ? 1 : 0, scratch.data_ptr());
    TORCH_CHECK(gxp != nullptr, "feature_l1: no low-resolution gradient");
    const int64_t off = reinterpret_cast<const char*>(gxp) - reinterpret_cast<const char*>(scratch.data_ptr());
    torch::Tensor gx = scratch.slice(0, off, off + (int64_t)Hg * Wg * C * 4).view(torch::kFloat32).view({Hg, Wg, C});
    return std::make_tuple(loss, d_fm, d_w, d_b, gx);
}

// forward-only resize -> 1x1 decoder (include/f3dgs.h: f3dgs_feature_decode); returns the (Cout, Hg, Wg) map, fp32 or fp16
torch::Tensor FeatureDecode(const torch::Tensor& feature_map, int64_t Hg, int64_t Wg, const torch::Tensor& weight,
                            const torch::Tensor& bias, bool half) {
    TORCH_CHECK(feature_map.is_cuda(), "feature_decode: tensors must live on a HIP device (no CPU path)");
    TORCH_CHECK(feature_map.dim() == 3, "feature_decode: feature_map (C,H,W) expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(feature_map.device());
    auto fm = dev_f32(feature_map, "feature_map");
    const bool dec = weight.numel() > 0;
    torch::Tensor w = weight, b = bias;
    const int C = fm.size(0), H = fm.size(1), W = fm.size(2);
    int Cout = C;
    if (dec) {
        w = dev_f32(weight, "weight");
        b = dev_f32(bias, "bias");
        TORCH_CHECK(w.dim() == 2 && w.size(1) == C && b.numel() == w.size(0), "feature_decode: weight (Cout,C) / bias (Cout) do not match feature_map");
        Cout = w.size(0);
    }
    torch::Tensor out = torch::empty({Cout, Hg, Wg}, fm.options().dtype(half ? torch::kFloat16 : torch::kFloat32));
    torch::Tensor scratch = torch::empty({(long long)f3dgs_feature_decode_scratch_bytes(C, (int)Hg, (int)Wg, dec ? 1 : 0)}, fm.options().dtype(torch::kByte));
    const int rc = f3dgs_feature_decode(C, H, W, Cout, (int)Hg, (int)Wg, fm.data_ptr<float>(), dec ? w.data_ptr<float>() : nullptr,
                                        dec ? b.data_ptr<float>() : nullptr, out.data_ptr(), half ? 1 : 0,
                                        dec ? scratch.data_ptr() : nullptr, current_stream(fm));
    check_status(rc, "feature_decode");
    return out;
}

// fused L1 + D-SSIM image loss (include/f3dgs.h: f3dgs_image_loss_forward); image and gt (C,H,W) or (N,C,H,W).  Returns
// (loss, l1, ssim, per-image ssim (N) or empty, scratch); with want_grad the scratch holds what image_loss_backward reads.
static void image_loss_check(const torch::Tensor& image, const torch::Tensor& gt) {
    TORCH_CHECK(image.is_cuda() && gt.is_cuda(), "image_loss: image and gt must live on a HIP device (no CPU path)");
    TORCH_CHECK(image.device() == gt.device(), "image_loss: image and gt are on different devices");
    TORCH_CHECK(image.scalar_type() == torch::kFloat32 && gt.scalar_type() == torch::kFloat32,
                "image_loss: image and gt must be float32 (got ", image.scalar_type(), ", ", gt.scalar_type(), ")");
    TORCH_CHECK(image.dim() == 3 || image.dim() == 4, "image_loss: a (C,H,W) or (N,C,H,W) image expected, got ", image.dim(), " dimensions");
    TORCH_CHECK(image.sizes() == gt.sizes(), "image_loss: image ", image.sizes(), " and gt ", gt.sizes(), " shapes differ");
    TORCH_CHECK(image.numel() > 0, "image_loss: empty image");
}

static std::array<int, 4> image_loss_dims(const torch::Tensor& t) {
    if (t.dim() == 3) return {1, (int)t.size(0), (int)t.size(1), (int)t.size(2)};
    return {(int)t.size(0), (int)t.size(1), (int)t.size(2), (int)t.size(3)};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
ImageLossForward(const torch::Tensor& image, const torch::Tensor& gt, double lambda_dssim, bool want_grad, bool per_image) {
    image_loss_check(image, gt);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(image.device());
    auto im = dev_f32(image, "image"), g = dev_f32(gt, "gt");
    const auto d = image_loss_dims(im);
    auto o = im.options();
    torch::Tensor loss = torch::empty({}, o), l1 = torch::empty({}, o), ssim = torch::empty({}, o);
    torch::Tensor ssim_img = per_image ? torch::empty({d[0]}, o) : torch::empty({0}, o);
    torch::Tensor scratch = torch::empty({(long long)f3dgs_image_loss_scratch_bytes(d[0], d[1], d[2], d[3], want_grad ? 1 : 0)},
                                         o.dtype(torch::kByte));
    const int rc = f3dgs_image_loss_forward(d[0], d[1], d[2], d[3], im.data_ptr<float>(), g.data_ptr<float>(), (float)lambda_dssim,
                                            want_grad ? 1 : 0, loss.data_ptr<float>(), l1.data_ptr<float>(), ssim.data_ptr<float>(),
                                            per_image ? ssim_img.data_ptr<float>() : nullptr, scratch.data_ptr(), current_stream(im));
    check_status(rc, "image_loss_forward");
    return std::make_tuple(loss, l1, ssim, ssim_img, scratch);
}

// the gradient with respect to `image` (include/f3dgs.h: f3dgs_image_loss_backward); `upstream` one value (modes 0, 1) or N
// (mode 2), on the device
torch::Tensor ImageLossBackward(const torch::Tensor& image, const torch::Tensor& gt, const torch::Tensor& scratch,
                                const torch::Tensor& upstream, double lambda_dssim, int64_t mode) {
    image_loss_check(image, gt);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(image.device());
    auto im = dev_f32(image, "image"), g = dev_f32(gt, "gt");
    const auto d = image_loss_dims(im);
    TORCH_CHECK(scratch.is_cuda() && scratch.is_contiguous() &&
                    scratch.numel() == (int64_t)f3dgs_image_loss_scratch_bytes(d[0], d[1], d[2], d[3], 1),
                "image_loss_backward: scratch is not what a want_grad forward call on this shape returned");
    auto u = dev_f32(upstream, "upstream");
    TORCH_CHECK(u.numel() == (mode == F3DGS_IMAGE_LOSS_SSIM_PER_IMAGE ? d[0] : 1), "image_loss_backward: upstream gradient of ",
                u.numel(), " values for mode ", mode);
    torch::Tensor d_image = torch::empty_like(im);
    const int rc = f3dgs_image_loss_backward(d[0], d[1], d[2], d[3], im.data_ptr<float>(), g.data_ptr<float>(), (float)lambda_dssim,
                                             (int)mode, u.data_ptr<float>(), scratch.data_ptr(), d_image.data_ptr<float>(),
                                             current_stream(im));
    check_status(rc, "image_loss_backward");
    return d_image;
}

// image-quality metrics of N view pairs (include/f3dgs.h: f3dgs_image_metrics).  image, gt: 4-D, float32 (N,C,H,W) for format
// F3DGS_IMAGE_F32, uint8 (N,C,H,W) or (N,H,W,C) for the two uint8 formats, each side by itself.  Returns (l1, mse, psnr, ssim),
// (N) float32 each; without want_ssim the last is empty and the windowed moments are not formed.
static std::array<int, 4> image_metrics_dims(const torch::Tensor& t, int64_t format, const char* name) {
    TORCH_CHECK(t.is_cuda(), "image_metrics: ", name, " must live on a HIP device (no CPU path)");
    TORCH_CHECK(t.dim() == 4, "image_metrics: ", name, " must have 4 dimensions, got ", t.dim());
    TORCH_CHECK(t.scalar_type() == (format == F3DGS_IMAGE_F32 ? torch::kFloat32 : torch::kByte), "image_metrics: ", name, " must be ",
                format == F3DGS_IMAGE_F32 ? "float32" : "uint8", " for format ", format);
    for (int i = 0; i < 4; i++) TORCH_CHECK(t.size(i) < (1ll << 31), "image_metrics: ", name, " is too large");
    if (format == F3DGS_IMAGE_U8_INTERLEAVED) return {(int)t.size(0), (int)t.size(3), (int)t.size(1), (int)t.size(2)};
    return {(int)t.size(0), (int)t.size(1), (int)t.size(2), (int)t.size(3)};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
ImageMetrics(const torch::Tensor& image, const torch::Tensor& gt, int64_t image_format, int64_t gt_format, int64_t flags, bool want_ssim) {
    const auto d = image_metrics_dims(image, image_format, "image"), dg = image_metrics_dims(gt, gt_format, "gt");
    TORCH_CHECK(d == dg, "image_metrics: image and gt shapes differ");
    TORCH_CHECK(image.device() == gt.device(), "image_metrics: image and gt are on different devices");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(image.device());
    const torch::Tensor im = image.contiguous(), g = gt.contiguous();
    auto o = im.options().dtype(torch::kFloat32);
    torch::Tensor l1 = torch::empty({d[0]}, o), mse = torch::empty({d[0]}, o), psnr = torch::empty({d[0]}, o);
    torch::Tensor ssim = torch::empty({want_ssim ? d[0] : 0}, o);
    if (d[0] == 0) return std::make_tuple(l1, mse, psnr, ssim);
    torch::Tensor scratch = torch::empty({(long long)f3dgs_image_metrics_scratch_bytes(d[0], d[1], d[2], d[3])}, o.dtype(torch::kByte));
    const int rc = f3dgs_image_metrics(d[0], d[1], d[2], d[3], im.data_ptr(), (int)image_format, g.data_ptr(), (int)gt_format, (int)flags,
                                       l1.data_ptr<float>(), mse.data_ptr<float>(), psnr.data_ptr<float>(),
                                       want_ssim ? ssim.data_ptr<float>() : nullptr, scratch.data_ptr(), current_stream(im));
    check_status(rc, "image_metrics");
    return std::make_tuple(l1, mse, psnr, ssim);
}

// segmentation scores of N view pairs (include/f3dgs.h: f3dgs_seg_metrics).  teacher, student, gt (empty: none): (N,H,W) uint8,
// int32 or int64, each by itself; a view at an odd storage offset is read where it lies.  carry_counts (A,L) / carry_scalars (5):
// the pooled counters of an earlier call, or empty.  Returns (counts (A,N+1,L) int64, scalars (5,N+1) int64, scores (2K,N+1)
// float64, iou_per_label (K,N+1,L) float64, labels_ranked (K,N+1,num_classes) int64); row N is the pooled one.  want_scores = false:
// the last three are empty and the finish kernel only pools the counters.
static int label_format(const torch::Tensor& t, const char* where, const char* name) {
    TORCH_CHECK(t.is_cuda(), where, ": ", name, " must live on a HIP device (no CPU path)");
    TORCH_CHECK(t.dim() == 3, where, ": ", name, " must be (N,H,W), got ", t.dim(), " dimensions");
    for (int i = 0; i < 3; i++) TORCH_CHECK(t.size(i) < (1ll << 31), where, ": ", name, " is too large");
    switch (t.scalar_type()) {
        case torch::kByte: return F3DGS_LABELS_U8;
        case torch::kInt32: return F3DGS_LABELS_I32;
        case torch::kInt64: return F3DGS_LABELS_I64;
        default: TORCH_CHECK(false, where, ": ", name, " must be uint8, int32 or int64, got ", t.scalar_type());
    }
    return -1;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
SegMetrics(const torch::Tensor& teacher, const torch::Tensor& student, const torch::Tensor& gt, int64_t L, int64_t num_classes,
           const torch::Tensor& carry_counts, const torch::Tensor& carry_scalars, bool want_scores) {
    const bool has_gt = gt.numel() != 0 || gt.dim() == 3;
    const int ft = label_format(teacher, "seg_metrics", "teacher"), fs = label_format(student, "seg_metrics", "student");
    const int fg = has_gt ? label_format(gt, "seg_metrics", "gt") : F3DGS_LABELS_U8;
    TORCH_CHECK(teacher.sizes() == student.sizes() && (!has_gt || gt.sizes() == teacher.sizes()), "seg_metrics: label map shapes differ");
    TORCH_CHECK(teacher.device() == student.device() && (!has_gt || gt.device() == teacher.device()),
                "seg_metrics: label maps are on different devices");
    TORCH_CHECK(L >= 1 && L <= F3DGS_SEGMENT_MAX_TEXTS, "seg_metrics: ", L, " label slots: 1 to ", F3DGS_SEGMENT_MAX_TEXTS, " are supported");
    TORCH_CHECK(num_classes >= 1 && num_classes <= L, "seg_metrics: num_classes ", num_classes, " outside 1..", L);
    const int64_t N = teacher.size(0), A = has_gt ? 7 : 3, K = has_gt ? 2 : 1;
    TORCH_CHECK(N >= 1 && teacher.size(1) >= 1 && teacher.size(2) >= 1, "seg_metrics: empty label maps ", teacher.sizes());
    const bool carry = carry_counts.numel() != 0;
    if (carry)
        TORCH_CHECK(carry_counts.is_cuda() && carry_scalars.is_cuda() && carry_counts.scalar_type() == torch::kInt64 &&
                        carry_scalars.scalar_type() == torch::kInt64 && carry_counts.numel() == A * L && carry_scalars.numel() == 5,
                    "seg_metrics: carry_counts (", A, ",", L, ") and carry_scalars (5) int64 device tensors expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(teacher.device());
    const torch::Tensor t = teacher.contiguous(), s = student.contiguous(), g = has_gt ? gt.contiguous() : gt;
    const torch::Tensor cc = carry ? carry_counts.contiguous() : carry_counts, cs = carry ? carry_scalars.contiguous() : carry_scalars;
    auto oi = t.options().dtype(torch::kInt64), od = t.options().dtype(torch::kFloat64);
    const int64_t count_words = A * (N + 1) * L;
    torch::Tensor block = torch::empty({(long long)(f3dgs_seg_metrics_scratch_bytes((int)N, (int)L, has_gt) / sizeof(int64_t))}, oi);
    TORCH_CHECK(block.numel() == count_words + 5 * (N + 1), "seg_metrics: unexpected counter block size");
    // without want_scores the three are empty and the library gets NULL: the counters alone (row N still pooled)
    const int64_t S = want_scores ? 1 : 0;
    torch::Tensor scores = torch::empty({S * 2 * K, N + 1}, od), per_label = torch::empty({S * K, N + 1, L}, od);
    torch::Tensor ranked = torch::empty({S * K, N + 1, num_classes}, oi);
    const int rc = f3dgs_seg_metrics((int)N, (int)t.size(1), (int)t.size(2), (int)L, (int)num_classes, t.data_ptr(), ft, s.data_ptr(), fs,
                                     has_gt ? g.data_ptr() : nullptr, fg, carry ? cc.data_ptr<int64_t>() : nullptr,
                                     carry ? cs.data_ptr<int64_t>() : nullptr, block.data_ptr<int64_t>(),
                                     want_scores ? scores.data_ptr<double>() : nullptr, want_scores ? per_label.data_ptr<double>() : nullptr,
                                     want_scores ? ranked.data_ptr<int64_t>() : nullptr, current_stream(t));
    check_status(rc, "seg_metrics");
    return std::make_tuple(block.narrow(0, 0, count_words).view({A, N + 1, L}), block.narrow(0, count_words, 5 * (N + 1)).view({5, N + 1}),
                           scores, per_label, ranked);
}

// palette pictures of label maps (include/f3dgs.h: f3dgs_seg_colorize).  labels (N,H,W) uint8 / int32 / int64, palette (L,3) uint8,
// image (N,3,H,W) float32 or empty (mask mode), fill: three byte values.  Returns uint8 (N,H,W',3), W' = 3 W for the strip.
torch::Tensor SegColorize(const torch::Tensor& labels, const torch::Tensor& palette, const torch::Tensor& image, int64_t mode, double a,
                          double b, const std::array<int, 3>& fill) {
    const int fl = label_format(labels, "seg_colorize", "labels");
    TORCH_CHECK(palette.is_cuda() && palette.device() == labels.device(), "seg_colorize: palette must live on the labels' device");
    TORCH_CHECK(palette.scalar_type() == torch::kByte && palette.dim() == 2 && palette.size(1) == 3 && palette.size(0) >= 1 &&
                    palette.size(0) <= F3DGS_SEGMENT_MAX_TEXTS,
                "seg_colorize: palette must be (L,3) uint8 with 1 <= L <= ", F3DGS_SEGMENT_MAX_TEXTS, ", got ", palette.sizes());
    TORCH_CHECK(mode == F3DGS_SEG_COLOR_MASK || mode == F3DGS_SEG_COLOR_BLEND || mode == F3DGS_SEG_COLOR_STRIP, "seg_colorize: unknown mode ", mode);
    const int64_t N = labels.size(0), H = labels.size(1), W = labels.size(2);
    TORCH_CHECK(N >= 1 && H >= 1 && W >= 1, "seg_colorize: empty label maps ", labels.sizes());
    const bool need_image = mode != F3DGS_SEG_COLOR_MASK;
    if (need_image)
        TORCH_CHECK(image.is_cuda() && image.device() == labels.device() && image.scalar_type() == torch::kFloat32 && image.dim() == 4 &&
                        image.size(0) == N && image.size(1) == 3 && image.size(2) == H && image.size(3) == W,
                    "seg_colorize: image must be float32 (", N, ",3,", H, ",", W, ") on the labels' device, got ", image.sizes());
    for (int v : fill) TORCH_CHECK(v >= 0 && v <= 255, "seg_colorize: fill must be three byte values");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(labels.device());
    const torch::Tensor l = labels.contiguous(), p = palette.contiguous(), im = need_image ? image.contiguous() : image;
    torch::Tensor out = torch::empty({N, H, mode == F3DGS_SEG_COLOR_STRIP ? 3 * W : W, 3}, l.options().dtype(torch::kByte));
    const unsigned char f[3] = {(unsigned char)fill[0], (unsigned char)fill[1], (unsigned char)fill[2]};
    const int rc = f3dgs_seg_colorize((int)N, (int)H, (int)W, (int)p.size(0), l.data_ptr(), fl, p.data_ptr<unsigned char>(),
                                      need_image ? im.data_ptr<float>() : nullptr, (int)mode, (float)a, (float)b, f,
                                      out.data_ptr<unsigned char>(), current_stream(l));
    check_status(rc, "seg_colorize");
    return out;
}

// SAM mask post-processing (include/f3dgs.h: f3dgs_sam_masks and what follows it; sam_masks.py checks the arguments and raises
// ValueError - the checks here guard the pointers).  low_res (M,h,w) float32, iou_preds (M) float32 or None.  Returns (packed
// (M,FW,ceil(FH/32)) int32, counts (M,3) int32, box (M,4) int32, box_frame (M,4) int32, stability (M) float32, keep (M) bool,
// kept_index (M) int32, kept_count (1) int32).
std::vector<torch::Tensor> SamMasks(const torch::Tensor& low_res, const c10::optional<torch::Tensor>& iou_preds, double pred_iou_thresh,
                                    int64_t S, int64_t ih, int64_t iw, int64_t H, int64_t W, int64_t FH, int64_t FW, int64_t cx0,
                                    int64_t cy0, double t, double t_hi, double t_lo, double stability_thresh, bool edge_filter) {
    TORCH_CHECK(low_res.is_cuda() && low_res.scalar_type() == torch::kFloat32 && low_res.dim() == 3,
                "sam_masks: low_res must be float32 (M,h,w) on a HIP device (no CPU path)");
    const int64_t M = low_res.size(0);
    TORCH_CHECK(FH >= 1 && FW >= 1 && FH <= 32768 && FW <= 32768 && M <= 65535, "sam_masks: bad frame or too many masks");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(low_res.device());
    const torch::Tensor lr = low_res.contiguous();
    torch::Tensor iou;
    if (iou_preds.has_value()) {
        TORCH_CHECK(iou_preds->is_cuda() && iou_preds->device() == low_res.device() && iou_preds->scalar_type() == torch::kFloat32 &&
                        iou_preds->numel() == M, "sam_masks: iou_preds must be ", M, " float32 values on low_res's device");
        iou = iou_preds->contiguous();
    }
    auto oi = lr.options().dtype(torch::kInt32);
    const int64_t NW = (FH + 31) / 32;
    torch::Tensor packed = torch::empty({M, FW, NW}, oi), counts = torch::empty({M, 3}, oi), box = torch::empty({M, 4}, oi);
    torch::Tensor box_frame = torch::empty({M, 4}, oi), stability = torch::empty({M}, lr.options()), keep = torch::empty({M}, oi.dtype(torch::kBool));
    torch::Tensor kept_index = torch::empty({M}, oi), kept_count = torch::empty({1}, oi);
    torch::Tensor scratch = torch::empty({(long long)f3dgs_sam_masks_scratch_bytes((int)M)}, oi.dtype(torch::kByte));
    const int rc = f3dgs_sam_masks((int)M, (int)lr.size(1), (int)lr.size(2), (int)S, (int)ih, (int)iw, (int)H, (int)W, (int)FH, (int)FW, (int)cx0,
                                   (int)cy0, M ? lr.data_ptr<float>() : nullptr, iou.defined() && M ? iou.data_ptr<float>() : nullptr,
                                   (float)pred_iou_thresh, (float)t, (float)t_hi, (float)t_lo, (float)stability_thresh, edge_filter ? 1 : 0,
                                   reinterpret_cast<uint32_t*>(packed.data_ptr()), counts.data_ptr<int32_t>(), box.data_ptr<int32_t>(),
                                   box_frame.data_ptr<int32_t>(), stability.data_ptr<float>(),
                                   reinterpret_cast<unsigned char*>(keep.data_ptr()), kept_index.data_ptr<int32_t>(),
                                   kept_count.data_ptr<int32_t>(), scratch.data_ptr(), current_stream(lr));
    check_status(rc, "sam_masks");
    return {packed, counts, box, box_frame, stability, keep, kept_index, kept_count};
}

// (M,H,W) float32 v, or bool v > t (f3dgs_sam_upscale)
torch::Tensor SamUpscale(const torch::Tensor& low_res, int64_t S, int64_t ih, int64_t iw, int64_t H, int64_t W, double t, bool out_bool) {
    TORCH_CHECK(low_res.is_cuda() && low_res.scalar_type() == torch::kFloat32 && low_res.dim() == 3,
                "sam_upscale: low_res must be float32 (M,h,w) on a HIP device (no CPU path)");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(low_res.device());
    const torch::Tensor lr = low_res.contiguous();
    const int64_t M = lr.size(0);
    TORCH_CHECK(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "sam_upscale: bad output size");
    torch::Tensor out = torch::empty({M, H, W}, lr.options().dtype(out_bool ? torch::kBool : torch::kFloat32));
    const int rc = f3dgs_sam_upscale((int)M, (int)lr.size(1), (int)lr.size(2), (int)S, (int)ih, (int)iw, (int)H, (int)W,
                                     M ? lr.data_ptr<float>() : nullptr, (float)t, out_bool ? 1 : 0, out.data_ptr(), current_stream(lr));
    check_status(rc, "sam_upscale");
    return out;
}

// SAM's prompt encoder and mask decoder (include/f3dgs.h: f3dgs_sam_decoder_*; sam_decoder.py checks names, shapes and the
// architecture and raises KeyError / ValueError / NotImplementedError - the checks here guard the pointers).
// params: F3DGS_SAM_DECODER_PARAMS contiguous float32 tensors on one HIP device, in the header's order -> the packed weights
torch::Tensor SamDecoderPack(const std::vector<torch::Tensor>& params) {
    TORCH_CHECK((int)params.size() == F3DGS_SAM_DECODER_PARAMS, "sam_decoder_pack: ", F3DGS_SAM_DECODER_PARAMS, " parameters expected, got ", params.size());
    std::vector<const float*> table;
    for (const torch::Tensor& p : params) {
        TORCH_CHECK(p.is_cuda() && p.device() == params[0].device() && p.scalar_type() == torch::kFloat32 && p.is_contiguous(),
                    "sam_decoder_pack: contiguous float32 parameters on one HIP device expected (no CPU path)");
        table.push_back(p.data_ptr<float>());
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params[0].device());
    torch::Tensor packed = torch::empty({(long long)(f3dgs_sam_decoder_weights_bytes() / sizeof(float))}, params[0].options());
    check_status(f3dgs_sam_decoder_pack_weights(table.data(), (int)table.size(), packed.data_ptr<float>(), current_stream(packed)), "sam_decoder_pack");
    return packed;
}

// features (256,h,w) float32 with any non-negative strides (read in place) -> the image plan
torch::Tensor SamDecoderPlan(const torch::Tensor& packed, const torch::Tensor& features) {
    TORCH_CHECK(features.is_cuda() && features.scalar_type() == torch::kFloat32 && features.dim() == 3,
                "sam_decoder_plan: features must be float32 (256,h,w) on a HIP device (no CPU path)");
    TORCH_CHECK(packed.is_cuda() && packed.device() == features.device() && packed.scalar_type() == torch::kFloat32 && packed.is_contiguous() &&
                    packed.numel() * sizeof(float) == f3dgs_sam_decoder_weights_bytes(), "sam_decoder_plan: packed weights on the features' device expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(features.device());
    const int h = (int)features.size(1), w = (int)features.size(2);
    const size_t bytes = f3dgs_sam_decoder_plan_bytes(h, w);
    torch::Tensor plan = torch::empty({(long long)(bytes / sizeof(float))}, packed.options());
    check_status(f3dgs_sam_decoder_plan((int)features.size(0), h, w, features.data_ptr<float>(), features.stride(0), features.stride(1), features.stride(2),
                                        packed.data_ptr<float>(), bytes ? plan.data_ptr<float>() : nullptr, current_stream(features)),
                 "sam_decoder_plan");
    return plan;
}

// coords (B,n,2) float32, labels (B,n) int32, boxes (B,4) float32 or None -> (low_res (B,m,4h,4w), iou (B,m)), m = 3 or 1
std::tuple<torch::Tensor, torch::Tensor> SamDecoderPredict(const torch::Tensor& plan, const torch::Tensor& packed, int64_t h, int64_t w,
                                                           const torch::Tensor& coords, const torch::Tensor& labels,
                                                           const c10::optional<torch::Tensor>& boxes, int64_t input_h, int64_t input_w, bool multimask) {
    TORCH_CHECK(plan.is_cuda() && packed.is_cuda() && plan.device() == packed.device() && plan.is_contiguous() && packed.is_contiguous(),
                "sam_decoder_predict: plan and packed weights on one HIP device expected");
    TORCH_CHECK(h >= 1 && w >= 1 && h * w <= F3DGS_SAM_DECODER_MAX_GRID && plan.numel() * sizeof(float) == f3dgs_sam_decoder_plan_bytes((int)h, (int)w) &&
                    packed.numel() * sizeof(float) == f3dgs_sam_decoder_weights_bytes(), "sam_decoder_predict: the plan is not one of an ", h, " x ", w, " grid");
    TORCH_CHECK(coords.device() == plan.device() && coords.scalar_type() == torch::kFloat32 && coords.dim() == 3 && coords.size(2) == 2 &&
                    coords.is_contiguous(), "sam_decoder_predict: coords must be contiguous float32 (B,n,2) on the plan's device");
    const int64_t B = coords.size(0), n = coords.size(1);
    TORCH_CHECK(labels.device() == plan.device() && labels.scalar_type() == torch::kInt32 && labels.dim() == 2 && labels.size(0) == B &&
                    labels.size(1) == n && labels.is_contiguous(), "sam_decoder_predict: labels must be contiguous int32 (B,n) on the plan's device");
    if (boxes)
        TORCH_CHECK(boxes->device() == plan.device() && boxes->scalar_type() == torch::kFloat32 && boxes->dim() == 2 && boxes->size(0) == B &&
                        boxes->size(1) == 4 && boxes->is_contiguous(), "sam_decoder_predict: boxes must be contiguous float32 (B,4) on the plan's device");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(plan.device());
    const int64_t m = multimask ? 3 : 1;
    torch::Tensor low_res = torch::empty({B, m, 4 * h, 4 * w}, plan.options()), iou = torch::empty({B, m}, plan.options());
    if (B == 0) return {low_res, iou};
    const int T = (int)(5 + n + (boxes ? 2 : 1));
    const size_t bytes = f3dgs_sam_decoder_scratch_bytes((int)B, (int)h, (int)w, T);
    torch::Tensor scratch = torch::empty({(long long)std::max<size_t>(bytes, 16)}, plan.options().dtype(torch::kByte));
    const int rc = f3dgs_sam_decoder_predict((int)B, (int)h, (int)w, (int)n, n ? coords.data_ptr<float>() : nullptr, n ? labels.data_ptr<int32_t>() : nullptr,
                                             boxes ? boxes->data_ptr<float>() : nullptr, (int)input_h, (int)input_w, multimask ? 1 : 0,
                                             plan.data_ptr<float>(), packed.data_ptr<float>(), low_res.data_ptr<float>(), iou.data_ptr<float>(),
                                             scratch.data_ptr(), bytes, current_stream(plan));
    check_status(rc, "sam_decoder_predict");
    return {low_res, iou};
}

// LPIPS, VGG16 (include/f3dgs.h: f3dgs_lpips_*; lpips_vgg.py checks names, shapes and arguments and raises KeyError / ValueError /
// NotImplementedError - the checks here guard the pointers).
// params: F3DGS_LPIPS_PARAMS contiguous float32 tensors on one HIP device, in the header's order -> the packed weights
torch::Tensor LpipsPack(const std::vector<torch::Tensor>& params) {
    TORCH_CHECK((int)params.size() == F3DGS_LPIPS_PARAMS, "lpips_pack: ", F3DGS_LPIPS_PARAMS, " parameters expected, got ", params.size());
    std::vector<const float*> table;
    for (const torch::Tensor& p : params) {
        TORCH_CHECK(p.is_cuda() && p.device() == params[0].device() && p.scalar_type() == torch::kFloat32 && p.is_contiguous(),
                    "lpips_pack: contiguous float32 parameters on one HIP device expected (no CPU path)");
        table.push_back(p.data_ptr<float>());
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params[0].device());
    torch::Tensor packed = torch::empty({(long long)(f3dgs_lpips_weights_bytes() / sizeof(float))}, params[0].options());
    check_status(f3dgs_lpips_pack_weights(table.data(), (int)table.size(), packed.data_ptr<float>(), current_stream(packed)), "lpips_pack");
    return packed;
}

static void lpips_check_image(const torch::Tensor& t, const torch::Tensor& packed, const char* where, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dim() == 4 && t.size(1) == 3 && (t.scalar_type() == torch::kFloat32 || t.scalar_type() == torch::kByte),
                where, ": ", name, " must be float32 or uint8 (N,3,H,W) on a HIP device (no CPU path)");
    TORCH_CHECK(packed.is_cuda() && packed.device() == t.device() && packed.scalar_type() == torch::kFloat32 && packed.is_contiguous() &&
                    packed.numel() * sizeof(float) == f3dgs_lpips_weights_bytes(), where, ": packed weights on the images' device expected");
    for (int d = 0; d < 4; d++) TORCH_CHECK(t.stride(d) >= 0, where, ": ", name, " has a negative stride");
}

int64_t LpipsWorkspaceBytes(int64_t N, int64_t H, int64_t W) { return (int64_t)f3dgs_lpips_workspace_bytes((int)N, (int)H, (int)W); }

// x, y (N,3,H,W) float32 or uint8 with any non-negative strides (read in place) -> (layer_terms (N,5), totals (N))
std::tuple<torch::Tensor, torch::Tensor> LpipsForward(const torch::Tensor& packed, const torch::Tensor& x, const torch::Tensor& y, int64_t flags) {
    lpips_check_image(x, packed, "lpips_forward", "x");
    lpips_check_image(y, packed, "lpips_forward", "y");
    TORCH_CHECK(x.sizes() == y.sizes() && x.device() == y.device(), "lpips_forward: x ", x.sizes(), " and y ", y.sizes(), " must agree, on one device");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    const int64_t N = x.size(0), H = x.size(2), W = x.size(3);
    torch::Tensor terms = torch::empty({N, 5}, packed.options()), totals = torch::empty({N}, packed.options());
    if (N == 0) return {terms, totals};
    const size_t bytes = f3dgs_lpips_workspace_bytes((int)N, (int)H, (int)W);
    TORCH_CHECK(bytes > 0, "lpips_forward: ", N, " pairs of ", H, " x ", W, " are not taken (H, W >= 16)");
    torch::Tensor ws = torch::empty({(long long)bytes}, packed.options().dtype(torch::kByte));
    const int rc = f3dgs_lpips_forward((int)N, (int)H, (int)W, x.data_ptr(), x.scalar_type() == torch::kByte ? F3DGS_LPIPS_U8 : F3DGS_LPIPS_F32,
                                       x.stride(0), x.stride(1), x.stride(2), x.stride(3), y.data_ptr(),
                                       y.scalar_type() == torch::kByte ? F3DGS_LPIPS_U8 : F3DGS_LPIPS_F32, y.stride(0), y.stride(1), y.stride(2),
                                       y.stride(3), (int)flags, packed.data_ptr<float>(), terms.data_ptr<float>(), totals.data_ptr<float>(),
                                       ws.data_ptr(), bytes, current_stream(x));
    check_status(rc, "lpips_forward");
    return {terms, totals};
}

// image (N,3,H,W) -> the five un-normalised taps (N,C_l,H_l,W_l)
std::vector<torch::Tensor> LpipsTaps(const torch::Tensor& packed, const torch::Tensor& image, bool quantize) {
    lpips_check_image(image, packed, "lpips_taps", "image");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(image.device());
    const int64_t N = image.size(0), H = image.size(2), W = image.size(3);
    static const int64_t C[5] = {64, 128, 256, 512, 512};
    std::vector<torch::Tensor> taps;
    std::vector<float*> table;
    for (int l = 0; l < 5; l++) {
        taps.push_back(torch::empty({N, C[l], H >> l, W >> l}, packed.options()));
        table.push_back(N ? taps[l].data_ptr<float>() : nullptr);
    }
    if (N == 0) return taps;
    const size_t bytes = f3dgs_lpips_workspace_bytes((int)((N + 1) / 2), (int)H, (int)W);
    TORCH_CHECK(bytes > 0, "lpips_taps: ", N, " images of ", H, " x ", W, " are not taken (H, W >= 16)");
    torch::Tensor ws = torch::empty({(long long)bytes}, packed.options().dtype(torch::kByte));
    const int rc = f3dgs_lpips_taps((int)N, (int)H, (int)W, image.data_ptr(), image.scalar_type() == torch::kByte ? F3DGS_LPIPS_U8 : F3DGS_LPIPS_F32,
                                    image.stride(0), image.stride(1), image.stride(2), image.stride(3), quantize ? 1 : 0, packed.data_ptr<float>(),
                                    table.data(), ws.data_ptr(), bytes, current_stream(image));
    check_status(rc, "lpips_taps");
    return taps;
}

// boxes (M,4) float32 IN SCORE ORDER, categories (M) int32 or None, order (M) int32 or None.  Returns (keep (M) int32, count (1) int32).
std::tuple<torch::Tensor, torch::Tensor> BoxNms(const torch::Tensor& boxes, const c10::optional<torch::Tensor>& categories,
                                                double iou_threshold, const c10::optional<torch::Tensor>& order) {
    TORCH_CHECK(boxes.is_cuda() && boxes.scalar_type() == torch::kFloat32 && boxes.dim() == 2 && boxes.size(1) == 4,
                "box_nms: boxes must be float32 (M,4) on a HIP device (no CPU path)");
    const int64_t M = boxes.size(0);
    TORCH_CHECK(M <= F3DGS_BOX_NMS_MAX, "box_nms: ", M, " boxes: up to ", F3DGS_BOX_NMS_MAX, " are supported");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(boxes.device());
    const torch::Tensor b = boxes.contiguous();
    torch::Tensor cat, ord;
    for (auto pr : {std::make_pair(&categories, &cat), std::make_pair(&order, &ord)})
        if (pr.first->has_value()) {
            const torch::Tensor& v = **pr.first;
            TORCH_CHECK(v.is_cuda() && v.device() == boxes.device() && v.scalar_type() == torch::kInt32 && v.numel() == M,
                        "box_nms: categories and order must be ", M, " int32 values on the boxes' device");
            *pr.second = v.contiguous();
        }
    auto oi = b.options().dtype(torch::kInt32);
    torch::Tensor keep = torch::empty({M}, oi), count = torch::empty({1}, oi);
    torch::Tensor scratch = torch::empty({(long long)(f3dgs_box_nms_scratch_bytes((int)M) / sizeof(int64_t))}, oi.dtype(torch::kInt64));
    const int rc = f3dgs_box_nms((int)M, M ? b.data_ptr<float>() : nullptr, cat.defined() && M ? cat.data_ptr<int32_t>() : nullptr,
                                 (float)iou_threshold, ord.defined() && M ? ord.data_ptr<int32_t>() : nullptr, keep.data_ptr<int32_t>(),
                                 count.data_ptr<int32_t>(), scratch.data_ptr(), current_stream(b));
    check_status(rc, "box_nms");
    return std::make_tuple(keep, count);
}

static void check_packed(const torch::Tensor& packed, const c10::optional<torch::Tensor>& index, int64_t FH, const char* where) {
    TORCH_CHECK(packed.is_cuda() && packed.scalar_type() == torch::kInt32 && packed.dim() == 3 && packed.is_contiguous() && FH >= 1 &&
                    packed.size(2) == (FH + 31) / 32 && packed.size(1) >= 1,
                where, ": packed must be contiguous int32 (M,FW,ceil(FH/32)) on a HIP device (no CPU path)");
    if (index.has_value())
        TORCH_CHECK(index->is_cuda() && index->device() == packed.device() && index->scalar_type() == torch::kInt32 && index->dim() == 1 &&
                        index->is_contiguous(), where, ": index must be contiguous int32 (K) on the masks' device");
}

// lens (K) int32 of the masks packed[index] (f3dgs_mask_rle_count)
torch::Tensor MaskRleCount(const torch::Tensor& packed, const c10::optional<torch::Tensor>& index, int64_t FH) {
    check_packed(packed, index, FH, "mask_rle_count");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(packed.device());
    const int64_t K = index.has_value() ? index->numel() : packed.size(0);
    torch::Tensor lens = torch::empty({K}, packed.options());
    const int rc = f3dgs_mask_rle_count((int)K, (int)FH, (int)packed.size(1), reinterpret_cast<const uint32_t*>(packed.data_ptr()),
                                        index.has_value() && K ? index->data_ptr<int32_t>() : nullptr, lens.data_ptr<int32_t>(),
                                        current_stream(packed));
    check_status(rc, "mask_rle_count");
    return lens;
}

// the counts of every mask into out[head + ends[k] - lens[k] ..), out (head + capacity) int32 (f3dgs_mask_rle_emit)
void MaskRleEmit(const torch::Tensor& packed, const c10::optional<torch::Tensor>& index, int64_t FH, const torch::Tensor& lens,
                 const torch::Tensor& ends, torch::Tensor& out, int64_t head) {
    check_packed(packed, index, FH, "mask_rle_emit");
    const int64_t K = index.has_value() ? index->numel() : packed.size(0);
    TORCH_CHECK(lens.is_cuda() && lens.scalar_type() == torch::kInt32 && lens.numel() == K && lens.is_contiguous() && ends.is_cuda() &&
                    ends.scalar_type() == torch::kInt64 && ends.numel() == K && ends.is_contiguous(),
                "mask_rle_emit: lens (K) int32 and ends (K) int64 expected");
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kInt32 && out.is_contiguous() && head >= 0 && out.numel() >= head,
                "mask_rle_emit: out must be contiguous int32 of at least `head` entries");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(packed.device());
    const int rc = f3dgs_mask_rle_emit((int)K, (int)FH, (int)packed.size(1), reinterpret_cast<const uint32_t*>(packed.data_ptr()),
                                       index.has_value() && K ? index->data_ptr<int32_t>() : nullptr, lens.data_ptr<int32_t>(),
                                       ends.data_ptr<int64_t>(), out.numel() - head, out.data_ptr<int32_t>() + head, current_stream(packed));
    check_status(rc, "mask_rle_emit");
}

// bool (K,FH,FW) (f3dgs_mask_unpack)
torch::Tensor MaskUnpack(const torch::Tensor& packed, const c10::optional<torch::Tensor>& index, int64_t FH) {
    check_packed(packed, index, FH, "mask_unpack");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(packed.device());
    const int64_t K = index.has_value() ? index->numel() : packed.size(0);
    torch::Tensor out = torch::empty({K, FH, packed.size(1)}, packed.options().dtype(torch::kBool));
    const int rc = f3dgs_mask_unpack((int)K, (int)FH, (int)packed.size(1), reinterpret_cast<const uint32_t*>(packed.data_ptr()),
                                     index.has_value() && K ? index->data_ptr<int32_t>() : nullptr,
                                     reinterpret_cast<unsigned char*>(out.data_ptr()), current_stream(packed));
    check_status(rc, "mask_unpack");
    return out;
}

// int32 (FH,FW): the largest j whose mask packed[index[j]] has the pixel set, -1 without one (f3dgs_mask_instance_map)
torch::Tensor MaskInstanceMap(const torch::Tensor& packed, const c10::optional<torch::Tensor>& index, int64_t FH) {
    check_packed(packed, index, FH, "mask_instance_map");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(packed.device());
    const int64_t K = index.has_value() ? index->numel() : packed.size(0);
    torch::Tensor out = torch::empty({FH, packed.size(1)}, packed.options());
    const int rc = f3dgs_mask_instance_map((int)K, (int)FH, (int)packed.size(1),
                                           K ? reinterpret_cast<const uint32_t*>(packed.data_ptr()) : nullptr,
                                           index.has_value() && K ? index->data_ptr<int32_t>() : nullptr, out.data_ptr<int32_t>(),
                                           current_stream(packed));
    check_status(rc, "mask_instance_map");
    return out;
}

// remove_small_regions of the masks packed[index] (f3dgs_mask_regions).  Returns (words (K,FW,NW) int32, changed (K) bool, area (K)
// int32, box (K,4) int32, runs): where runs > run_capacity the tensors are unwritten and the caller comes again.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, int64_t>
MaskRegions(const torch::Tensor& packed, const c10::optional<torch::Tensor>& index, int64_t FH, double area_thresh, bool holes,
            int64_t run_capacity) {
    check_packed(packed, index, FH, "mask_regions");
    TORCH_CHECK(run_capacity >= 0 && run_capacity <= 2147483647LL, "mask_regions: run_capacity out of range");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(packed.device());
    const int64_t K = index.has_value() ? index->numel() : packed.size(0);
    const int64_t FW = packed.size(1);
    TORCH_CHECK(K <= 65535 && FH <= 32768 && FW <= 32768, "mask_regions: up to 65535 masks of up to 32768 a side are supported");
    auto oi = packed.options();
    torch::Tensor out = torch::empty({K, FW, packed.size(2)}, oi), changed = torch::empty({K}, oi.dtype(torch::kBool));
    torch::Tensor area = torch::empty({K}, oi), box = torch::empty({K, 4}, oi);
    torch::Tensor scratch = torch::empty({(long long)((f3dgs_mask_regions_scratch_bytes((int)K, (int)FW, run_capacity) + 7) / 8)}, oi.dtype(torch::kInt64));
    int64_t runs = 0;
    const int rc = f3dgs_mask_regions((int)K, (int)FH, (int)FW, reinterpret_cast<const uint32_t*>(packed.data_ptr()),
                                      index.has_value() && K ? index->data_ptr<int32_t>() : nullptr, holes ? 1 : 0, area_thresh, run_capacity,
                                      reinterpret_cast<uint32_t*>(out.data_ptr()), reinterpret_cast<unsigned char*>(changed.data_ptr()),
                                      area.data_ptr<int32_t>(), box.data_ptr<int32_t>(), &runs, scratch.data_ptr(), current_stream(packed));
    check_status(rc, "mask_regions");
    return std::make_tuple(out, changed, area, box, runs);
}

// language-guided selection (include/f3dgs.h: f3dgs_edit_select).  features (P, C) float32, contiguous and 16-byte aligned where
// normalize_inplace asks for the write-back (edit.py copies other views and copies back); text (K, C).  Returns (mask (P),
// score (P) or None, opacity_out like opacity or None).
std::tuple<torch::Tensor, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
EditSelect(torch::Tensor& features, const torch::Tensor& text, uint64_t positive_mask, int64_t first_positive, int64_t variant,
           const c10::optional<double>& threshold, bool normalize_inplace, bool want_score,
           const c10::optional<torch::Tensor>& opacity) {
    TORCH_CHECK(features.is_cuda() && text.is_cuda(), "edit_select: features and text must live on a HIP device (no CPU path)");
    TORCH_CHECK(features.device() == text.device(), "edit_select: features and text are on different devices");
    TORCH_CHECK(features.scalar_type() == torch::kFloat32 && text.scalar_type() == torch::kFloat32,
                "edit_select: features and text must be float32 (got ", features.scalar_type(), ", ", text.scalar_type(), ")");
    TORCH_CHECK(features.dim() == 2 && text.dim() == 2 && features.size(1) == text.size(1) && text.size(0) >= 1 && text.size(1) >= 1,
                "edit_select: features (P, C) and text (K, C) expected, got ", features.sizes(), " and ", text.sizes());
    TORCH_CHECK(features.size(0) <= (1 << 30), "edit_select: too many rows");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(features.device());
    torch::Tensor f = features;
    if (normalize_inplace) {
        TORCH_CHECK(features.is_contiguous(), "edit_select: normalize_inplace needs contiguous features");
    } else {
        f = features.contiguous();
    }
    const torch::Tensor t = text.contiguous();
    const int P = (int)f.size(0), C = (int)f.size(1), K = (int)t.size(0);
    auto o = f.options();
    torch::Tensor mask = torch::empty({P}, o);
    c10::optional<torch::Tensor> score, op_out;
    if (want_score) score = torch::empty({P}, o);
    torch::Tensor op_in;
    if (opacity.has_value()) {
        TORCH_CHECK(opacity->is_cuda() && opacity->scalar_type() == torch::kFloat32 && opacity->numel() == P,
                    "edit_select: opacity must be ", P, " float32 values on the device");
        op_in = opacity->contiguous();
        op_out = torch::empty_like(op_in);
    }
    const int rc = f3dgs_edit_select(P, C, K, fptr(f), normalize_inplace ? f.data_ptr<float>() : nullptr, t.data_ptr<float>(),
                                     positive_mask, (int)first_positive, (int)variant, threshold.has_value() ? 1 : 0,
                                     threshold.has_value() ? (float)*threshold : 0.f, P ? mask.data_ptr<float>() : nullptr,
                                     (want_score && P) ? score->data_ptr<float>() : nullptr,
                                     (op_out.has_value() && P) ? op_in.data_ptr<float>() : nullptr,
                                     (op_out.has_value() && P) ? op_out->data_ptr<float>() : nullptr, current_stream(f));
    check_status(rc, "edit_select");
    return std::make_tuple(mask, score, op_out);
}

// What the operators over the state buffers of a rasterize_gaussians call (contributions, label_votes; `op` names one in the
// messages) check alike: the buffers and the sizes ...
void check_walk_state(const char* op, const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imgBuffer,
                      int64_t P, int64_t H, int64_t W) {
    TORCH_CHECK(imgBuffer.is_cuda() && geomBuffer.is_cuda() && binningBuffer.is_cuda(), op,
                ": the state buffers must live on a HIP device (no CPU path)");
    TORCH_CHECK(P >= 0 && H > 0 && W > 0 && H * W < (1ll << 31), op, ": bad sizes P = ", P, ", image ", H, " x ", W);
}
// ... and that an operand lives where they do
void check_on_state_device(const char* op, const torch::Tensor& t, const char* name, const torch::Device& dev) {
    TORCH_CHECK(t.is_cuda() && t.device() == dev, op, ": ", name, " must live on the HIP device of the state buffers (got ", t.device(), ")");
}
// a state buffer as the library takes it (an empty one: null)
const char* state_ptr(const torch::Tensor& t) { return t.numel() ? reinterpret_cast<const char*>(t.data_ptr()) : nullptr; }

// the contribution pass (include/f3dgs.h: f3dgs_contributions) over the state buffers of a rasterize_gaussians call: masks
// (K, H, W) float32 or None; acc (P, K + 1) float32, added to, or None; wmax (P) float32, max-ed into, or None; want_pixel: the
// four per-pixel outputs.  Returns (alpha, median_depth, ids, id_weight), each (H, W), or four None.
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
Contributions(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imgBuffer, int64_t P,
              int64_t num_rendered, int64_t H, int64_t W, const c10::optional<torch::Tensor>& masks, c10::optional<torch::Tensor> acc,
              c10::optional<torch::Tensor> wmax, bool want_pixel) {
    check_walk_state("contributions", geomBuffer, binningBuffer, imgBuffer, P, H, W);
    const auto dev = imgBuffer.device();
    auto on_dev_f32 = [&](const torch::Tensor& t, const char* name) {
        check_on_state_device("contributions", t, name, dev);
        TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.is_contiguous(), "contributions: ", name, " must be contiguous float32");
    };
    int64_t K = 0;
    if (masks.has_value()) {
        on_dev_f32(*masks, "masks");
        TORCH_CHECK(masks->dim() == 3 && masks->size(1) == H && masks->size(2) == W, "contributions: masks (K, ", H, ", ", W,
                    ") expected, got ", masks->sizes());
        K = masks->size(0);
        TORCH_CHECK(K <= F3DGS_CONTRIB_MAX_MASKS, "contributions: ", K, " masks, at most ", F3DGS_CONTRIB_MAX_MASKS, " per call");
        TORCH_CHECK(K == 0 || acc.has_value(), "contributions: masks without acc");
    }
    if (acc.has_value()) {
        on_dev_f32(*acc, "acc");
        TORCH_CHECK(acc->dim() == 2 && acc->size(0) == P && acc->size(1) == K + 1, "contributions: acc (", P, ", ", K + 1,
                    ") expected, got ", acc->sizes());
    }
    if (wmax.has_value()) {
        on_dev_f32(*wmax, "wmax");
        TORCH_CHECK(wmax->dim() == 1 && wmax->size(0) == P, "contributions: wmax (", P, ") expected, got ", wmax->sizes());
    }
    TORCH_CHECK(acc.has_value() || wmax.has_value() || want_pixel, "contributions: no output asked for");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    c10::optional<torch::Tensor> alpha, median, ids, id_weight;
    if (want_pixel) {
        auto f32 = imgBuffer.options().dtype(torch::kFloat32);
        alpha = torch::empty({H, W}, f32);
        median = torch::empty({H, W}, f32);
        ids = torch::empty({H, W}, imgBuffer.options().dtype(torch::kInt32));
        id_weight = torch::empty({H, W}, f32);
    }
    const bool per_gaussian = P > 0;      // (P, .) tensors of no rows have no storage: nothing to add to
    if (!per_gaussian) K = 0;
    if (!per_gaussian && !want_pixel) return std::make_tuple(alpha, median, ids, id_weight);
    const int rc = f3dgs_contributions(
        (int)P, (int)num_rendered, (int)W, (int)H, state_ptr(geomBuffer), state_ptr(binningBuffer), state_ptr(imgBuffer), (int)K,
        K ? masks->data_ptr<float>() : nullptr, (acc.has_value() && per_gaussian) ? acc->data_ptr<float>() : nullptr,
        (wmax.has_value() && per_gaussian) ? wmax->data_ptr<float>() : nullptr, want_pixel ? alpha->data_ptr<float>() : nullptr,
        want_pixel ? median->data_ptr<float>() : nullptr, want_pixel ? ids->data_ptr<int>() : nullptr,
        want_pixel ? id_weight->data_ptr<float>() : nullptr, current_stream(imgBuffer));
    check_status(rc, "contributions");
    return std::make_tuple(alpha, median, ids, id_weight);
}

// the label vote (include/f3dgs.h: f3dgs_label_votes) over the state buffers of a rasterize_gaussians call: labels (H, W) uint8 /
// int32 / int64; acc (P, L + 1) float32, added to
void LabelVotes(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer, const torch::Tensor& imgBuffer, int64_t P,
                int64_t num_rendered, int64_t H, int64_t W, const torch::Tensor& labels, int64_t L, torch::Tensor& acc) {
    check_walk_state("label_votes", geomBuffer, binningBuffer, imgBuffer, P, H, W);
    TORCH_CHECK(L >= 1 && L <= F3DGS_LABEL_VOTES_MAX_LABELS, "label_votes: L = ", L, " labels, 1 .. ", F3DGS_LABEL_VOTES_MAX_LABELS, " are taken");
    const auto dev = imgBuffer.device();
    const auto st = labels.scalar_type();
    check_on_state_device("label_votes", labels, "labels", dev);
    TORCH_CHECK((st == torch::kUInt8 || st == torch::kInt32 || st == torch::kInt64) && labels.is_contiguous() && labels.dim() == 2 &&
                    labels.size(0) == H && labels.size(1) == W,
                "label_votes: labels must be contiguous uint8, int32 or int64 (", H, ", ", W, "), got ", st, " ", labels.sizes());
    TORCH_CHECK(acc.is_cuda() && acc.device() == dev && acc.scalar_type() == torch::kFloat32 && acc.is_contiguous() && acc.dim() == 2 &&
                    acc.size(0) == P && acc.size(1) == L + 1,
                "label_votes: acc must be contiguous float32 (", P, ", ", L + 1, ") on the device of the state buffers, got ", acc.sizes());
    if (P == 0) return;      // a (0, .) tensor has no storage: nothing to add to
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const int format = st == torch::kUInt8 ? F3DGS_LABELS_U8 : st == torch::kInt32 ? F3DGS_LABELS_I32 : F3DGS_LABELS_I64;
    const int rc = f3dgs_label_votes((int)P, (int)num_rendered, (int)W, (int)H, state_ptr(geomBuffer), state_ptr(binningBuffer),
                                     state_ptr(imgBuffer), labels.data_ptr(), format, (int)L, acc.data_ptr<float>(), current_stream(imgBuffer));
    check_status(rc, "label_votes");
}

// What instance_associate and instance_merge (`op` names one in the messages) check alike: acc_view (P, M + 1) and acc (P, L + 1),
// contiguous float32 on one HIP device.  Returns (P, M, L).
std::tuple<int64_t, int64_t, int64_t> check_instance_votes(const char* op, const torch::Tensor& acc_view, const torch::Tensor& acc) {
    TORCH_CHECK(acc_view.is_cuda() && acc.is_cuda(), op, ": acc_view and acc must live on a HIP device (no CPU path)");
    TORCH_CHECK(acc.device() == acc_view.device(), op, ": acc on ", acc.device(), ", acc_view on ", acc_view.device());
    TORCH_CHECK(acc_view.scalar_type() == torch::kFloat32 && acc_view.is_contiguous() && acc_view.dim() == 2 && acc_view.size(1) >= 2, op,
                ": acc_view must be contiguous float32 (P, M + 1), got ", acc_view.scalar_type(), " ", acc_view.sizes());
    TORCH_CHECK(acc.scalar_type() == torch::kFloat32 && acc.is_contiguous() && acc.dim() == 2 && acc.size(1) >= 2 && acc.size(0) == acc_view.size(0),
                op, ": acc must be contiguous float32 (", acc_view.size(0), ", L + 1), got ", acc.scalar_type(), " ", acc.sizes());
    const int64_t P = acc_view.size(0), M = acc_view.size(1) - 1, L = acc.size(1) - 1;
    TORCH_CHECK(P < (1ll << 31), op, ": P = ", P, " rows");
    TORCH_CHECK(M <= F3DGS_INSTANCE_MAX_MASKS, op, ": M = ", M, " masks, 1 .. ", F3DGS_INSTANCE_MAX_MASKS, " are taken");
    TORCH_CHECK(L <= F3DGS_INSTANCE_MAX_INSTANCES, op, ": L = ", L, " instances, 1 .. ", F3DGS_INSTANCE_MAX_INSTANCES, " are taken");
    return std::make_tuple(P, M, L);
}

// association of a view's masks with the 3D instances (include/f3dgs.h: f3dgs_instance_associate).  count, dropped: int32 tensors
// of one element on the device, updated in place.  Returns (mapping (M) int32, best_label (M) int32, best_iou (M) float64,
// table (M + 1, L + 1) float32).
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
InstanceAssociate(const torch::Tensor& acc_view, const torch::Tensor& acc, torch::Tensor& count, torch::Tensor& dropped, double iou_thresh,
                  double min_weight) {
    int64_t P, M, L;
    std::tie(P, M, L) = check_instance_votes("instance_associate", acc_view, acc);
    const auto dev = acc_view.device();
    auto counter = [&](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == torch::kInt32 && t.numel() == 1 && t.is_contiguous(),
                    "instance_associate: ", name, " must be one int32 on the device of acc_view, got ", t.scalar_type(), " ", t.sizes(), " on ",
                    t.device());
    };
    counter(count, "count");
    counter(dropped, "dropped");
    TORCH_CHECK(iou_thresh >= 0.0 && min_weight >= 0.0, "instance_associate: iou_thresh and min_weight must be >= 0 (got ", iou_thresh, ", ",
                min_weight, ")");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    auto i32 = acc_view.options().dtype(torch::kInt32);
    torch::Tensor mapping = torch::empty({M}, i32), best_label = torch::empty({M}, i32);
    torch::Tensor best_iou = torch::empty({M}, acc_view.options().dtype(torch::kFloat64));
    torch::Tensor table = torch::empty({M + 1, L + 1}, acc_view.options());
    torch::Tensor scratch = torch::empty({(long long)f3dgs_instance_scratch_bytes((int)M, (int)L)}, acc_view.options().dtype(torch::kByte));
    const int rc = f3dgs_instance_associate((int)P, (int)M, (int)L, P ? acc_view.data_ptr<float>() : nullptr, P ? acc.data_ptr<float>() : nullptr,
                                            iou_thresh, min_weight, count.data_ptr<int>(), dropped.data_ptr<int>(), mapping.data_ptr<int>(),
                                            best_label.data_ptr<int>(), best_iou.data_ptr<double>(), table.data_ptr<float>(),
                                            scratch.data_ptr(), current_stream(acc_view));
    check_status(rc, "instance_associate");
    return std::make_tuple(mapping, best_label, best_iou, table);
}

// the merge under a mapping (include/f3dgs.h: f3dgs_instance_merge): acc is added to; acc_view is cleared where it was read as
// non-zero with clear_view
void InstanceMerge(torch::Tensor& acc_view, const torch::Tensor& mapping, torch::Tensor& acc, bool clear_view) {
    int64_t P, M, L;
    std::tie(P, M, L) = check_instance_votes("instance_merge", acc_view, acc);
    TORCH_CHECK(mapping.is_cuda() && mapping.device() == acc_view.device() && mapping.scalar_type() == torch::kInt32 && mapping.is_contiguous() &&
                    mapping.dim() == 1 && mapping.size(0) == M,
                "instance_merge: mapping must be contiguous int32 (", M, ") on the device of acc_view, got ", mapping.scalar_type(), " ",
                mapping.sizes(), " on ", mapping.device());
    if (P == 0) return;      // a (0, .) tensor has no storage: nothing to add to
    c10::hip::HIPGuardMasqueradingAsCUDA guard(acc_view.device());
    const int rc = f3dgs_instance_merge((int)P, (int)M, (int)L, acc_view.data_ptr<float>(), clear_view ? 1 : 0, mapping.data_ptr<int>(),
                                        acc.data_ptr<float>(), current_stream(acc_view));
    check_status(rc, "instance_merge");
}

// open-vocabulary segmentation (include/f3dgs.h: f3dgs_segment).  feature_map (C,H,W), text (K,Cout) float32; weight (Cout,C) /
// bias (Cout) or empty tensors.  Returns (labels (Hs,Ws) int64, score (Hs,Ws) float32 or None).
std::tuple<torch::Tensor, c10::optional<torch::Tensor>>
Segment(const torch::Tensor& feature_map, const torch::Tensor& text, int64_t Hs, int64_t Ws, const torch::Tensor& weight,
        const torch::Tensor& bias, int64_t flags, bool want_score) {
    TORCH_CHECK(feature_map.is_cuda() && text.is_cuda(), "segment: feature_map and text must live on a HIP device (no CPU path)");
    TORCH_CHECK(feature_map.device() == text.device(), "segment: feature_map and text are on different devices");
    TORCH_CHECK(feature_map.scalar_type() == torch::kFloat32 && text.scalar_type() == torch::kFloat32,
                "segment: feature_map and text must be float32 (got ", feature_map.scalar_type(), ", ", text.scalar_type(), ")");
    TORCH_CHECK(feature_map.dim() == 3 && text.dim() == 2, "segment: feature_map (C,H,W) and text (K,Cout) expected");
    TORCH_CHECK(Hs >= 0 && Ws >= 0 && Hs * Ws <= (1ll << 30), "segment: bad output size");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(feature_map.device());
    auto fm = feature_map.contiguous(), t = text.contiguous();
    const bool dec = weight.numel() > 0;
    torch::Tensor w = weight, b = bias;
    const int C = fm.size(0), H = fm.size(1), W = fm.size(2), K = t.size(0);
    int Cout = C;
    if (dec) {
        w = dev_f32(weight, "weight");
        b = dev_f32(bias, "bias");
        TORCH_CHECK(w.dim() == 2 && w.size(1) == C && b.numel() == w.size(0), "segment: weight (Cout,C) / bias (Cout) do not match feature_map");
        Cout = w.size(0);
    }
    TORCH_CHECK(t.size(1) == Cout, "segment: text has ", t.size(1), " channels, the scored map ", Cout);
    torch::Tensor labels = torch::empty({Hs, Ws}, fm.options().dtype(torch::kInt64));
    c10::optional<torch::Tensor> score;
    if (want_score) score = torch::empty({Hs, Ws}, fm.options());
    torch::Tensor scratch = torch::empty({(long long)f3dgs_segment_scratch_bytes(C, Cout, (int)Hs, (int)Ws, K, dec ? 1 : 0)},
                                         fm.options().dtype(torch::kByte));
    const bool any = Hs * Ws > 0;
    const int rc = f3dgs_segment(C, H, W, Cout, (int)Hs, (int)Ws, K, fm.data_ptr<float>(), dec ? w.data_ptr<float>() : nullptr,
                                 dec ? b.data_ptr<float>() : nullptr, t.data_ptr<float>(), (int)flags,
                                 any ? labels.data_ptr<int64_t>() : nullptr, (want_score && any) ? score->data_ptr<float>() : nullptr,
                                 scratch.data_ptr(), current_stream(fm));
    check_status(rc, "segment");
    return std::make_tuple(labels, score);
}

// PCA of a feature map (include/f3dgs.h: f3dgs_feature_pca_*).  feature_map (C,H,W) float32.  Returns (mean (C), cov (C,C)) float64.
std::tuple<torch::Tensor, torch::Tensor> FeaturePcaMoments(const torch::Tensor& feature_map, int64_t stride) {
    TORCH_CHECK(feature_map.is_cuda(), "feature_pca_moments: feature_map must live on a HIP device (no CPU path)");
    TORCH_CHECK(feature_map.scalar_type() == torch::kFloat32 && feature_map.dim() == 3, "feature_pca_moments: feature_map (C,H,W) float32 expected");
    TORCH_CHECK(stride >= 1 && stride <= (1ll << 30), "feature_pca_moments: bad stride");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(feature_map.device());
    auto fm = feature_map.contiguous();
    const int C = (int)fm.size(0);
    const long long HW = fm.size(1) * fm.size(2);
    auto o = fm.options().dtype(torch::kFloat64);
    torch::Tensor mean = torch::empty({C}, o), cov = torch::empty({C, C}, o);
    torch::Tensor scratch = torch::empty({(long long)f3dgs_feature_pca_scratch_bytes(C, HW, (int)stride)}, fm.options().dtype(torch::kByte));
    check_status(f3dgs_feature_pca_moments(C, HW, (int)stride, fptr(fm), mean.data_ptr<double>(), cov.data_ptr<double>(),
                                           scratch.data_ptr(), current_stream(fm)),
                 "feature_pca_moments");
    return std::make_tuple(mean, cov);
}

// mean (C), components (3,C) float32; lo / hi 0-dim float32 device tensors or None.  Returns (H,W,3) float32.
torch::Tensor FeaturePcaProject(const torch::Tensor& feature_map, const torch::Tensor& mean, const torch::Tensor& components,
                                const c10::optional<torch::Tensor>& lo, const c10::optional<torch::Tensor>& hi) {
    TORCH_CHECK(feature_map.is_cuda(), "feature_pca_project: feature_map must live on a HIP device (no CPU path)");
    TORCH_CHECK(feature_map.scalar_type() == torch::kFloat32 && feature_map.dim() == 3, "feature_pca_project: feature_map (C,H,W) float32 expected");
    TORCH_CHECK(lo.has_value() == hi.has_value(), "feature_pca_project: lo and hi go together");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(feature_map.device());
    auto fm = feature_map.contiguous();
    const int C = (int)fm.size(0);
    const long long H = fm.size(1), W = fm.size(2);
    auto dev = [&](const torch::Tensor& t, long long numel, const char* what) {
        TORCH_CHECK(t.is_cuda() && t.device() == fm.device() && t.scalar_type() == torch::kFloat32 && t.numel() == numel,
                    "feature_pca_project: ", what, " must be ", numel, " float32 value(s) on the map's device");
        return t.contiguous();
    };
    const torch::Tensor m = dev(mean, C, "mean"), comp = dev(components, 3ll * C, "components");
    torch::Tensor l, h;
    if (lo.has_value()) { l = dev(*lo, 1, "lo"); h = dev(*hi, 1, "hi"); }
    torch::Tensor out = torch::empty({H, W, 3}, fm.options());
    check_status(f3dgs_feature_pca_project(C, H * W, fptr(fm), m.data_ptr<float>(), comp.data_ptr<float>(),
                                           lo.has_value() ? l.data_ptr<float>() : nullptr, lo.has_value() ? h.data_ptr<float>() : nullptr,
                                           H * W ? out.data_ptr<float>() : nullptr, current_stream(fm)),
                 "feature_pca_project");
    return out;
}

// The viewer's render modes (include/f3dgs.h: f3dgs_view_*).  Shapes are view_modes.py's to check; here: device, dtype, sizes.
static torch::Tensor view_f32(const torch::Tensor& t, const char* what) {
    TORCH_CHECK(t.is_cuda(), "view_modes: ", what, " must live on a HIP device (no CPU path)");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, "view_modes: ", what, " must be float32");
    return t.contiguous();
}

struct ViewCamera {
    torch::Tensor proj, inv;
    ViewCamera(const torch::Tensor& depth, const torch::Tensor& projection, const torch::Tensor& inv_full_proj) {
        proj = view_f32(projection, "projection_matrix");
        TORCH_CHECK(inv_full_proj.is_cuda() && inv_full_proj.scalar_type() == torch::kFloat64,
                    "view_modes: the inverse of full_proj_transform must be float64 on a HIP device");
        inv = inv_full_proj.contiguous();
        TORCH_CHECK(proj.numel() == 16 && inv.numel() == 16, "view_modes: 4 x 4 matrices expected");
        TORCH_CHECK(proj.device() == depth.device() && inv.device() == depth.device(), "view_modes: the matrices must live on the depth map's device");
    }
};

// depth (H,W) float32.  Returns (H,W,3), or (3,H,W) with chw; with half the values are (n + 1) / 2.
torch::Tensor ViewNormals(const torch::Tensor& depth, const torch::Tensor& projection, const torch::Tensor& inv_full_proj, bool chw,
                          bool half) {
    auto d = view_f32(depth, "depth");
    TORCH_CHECK(d.dim() == 2, "view_normals: depth (H,W) expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(d.device());
    const ViewCamera cam(d, projection, inv_full_proj);
    const long long H = d.size(0), W = d.size(1);
    TORCH_CHECK(H * W <= (1ll << 30), "view_normals: the frame is too large");
    torch::Tensor out = chw ? torch::empty({3, H, W}, d.options()) : torch::empty({H, W, 3}, d.options());
    check_status(f3dgs_view_normals((int)H, (int)W, fptr(d), cam.proj.data_ptr<float>(), cam.inv.data_ptr<double>(),
                                    H * W ? out.data_ptr<float>() : nullptr,
                                    (chw ? F3DGS_VIEW_NORMALS_CHW : 0) | (half ? F3DGS_VIEW_NORMALS_HALF : 0), current_stream(d)),
                 "view_normals");
    return out;
}

// image (Cn,H,W) float32.  Returns (field (H,W), minmax (2)).
std::tuple<torch::Tensor, torch::Tensor> ViewGradient(const torch::Tensor& image) {
    auto im = view_f32(image, "image");
    TORCH_CHECK(im.dim() == 3 && im.size(0) >= 1, "view_gradient: image (Cn,H,W) with Cn >= 1 expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(im.device());
    const long long H = im.size(1), W = im.size(2);
    TORCH_CHECK(H * W <= (1ll << 30) && im.size(0) <= (1ll << 30), "view_gradient: the image is too large");
    torch::Tensor out = torch::empty({H, W}, im.options()), minmax = torch::empty({2}, im.options());
    check_status(f3dgs_view_gradient((int)im.size(0), (int)H, (int)W, fptr(im), H * W ? out.data_ptr<float>() : nullptr,
                                     minmax.data_ptr<float>(), current_stream(im)),
                 "view_gradient");
    return std::make_tuple(out, minmax);
}

std::tuple<torch::Tensor, torch::Tensor> ViewCurvature(const torch::Tensor& depth, const torch::Tensor& projection,
                                                       const torch::Tensor& inv_full_proj) {
    auto d = view_f32(depth, "depth");
    TORCH_CHECK(d.dim() == 2, "view_curvature: depth (H,W) expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(d.device());
    const ViewCamera cam(d, projection, inv_full_proj);
    const long long H = d.size(0), W = d.size(1);
    TORCH_CHECK(H * W <= (1ll << 30), "view_curvature: the frame is too large");
    torch::Tensor out = torch::empty({H, W}, d.options()), minmax = torch::empty({2}, d.options());
    check_status(f3dgs_view_curvature((int)H, (int)W, fptr(d), cam.proj.data_ptr<float>(), cam.inv.data_ptr<double>(),
                                      H * W ? out.data_ptr<float>() : nullptr, minmax.data_ptr<float>(), current_stream(d)),
                 "view_curvature");
    return std::make_tuple(out, minmax);
}

torch::Tensor ViewMinmax(const torch::Tensor& field) {
    auto f = view_f32(field, "field");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(f.device());
    torch::Tensor minmax = torch::empty({2}, f.options());
    check_status(f3dgs_view_minmax(f.numel(), fptr(f), minmax.data_ptr<float>(), current_stream(f)), "view_minmax");
    return minmax;
}

// field: any shape of HW float32 values; minmax (2), lut (L,3).  Returns ((3, *field.shape) float32 or None, (*field.shape, 3)
// uint8 or None).
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>> ViewPalette(const torch::Tensor& field, const torch::Tensor& minmax,
                                                                                    const torch::Tensor& lut, int64_t mode, bool want_float,
                                                                                    bool want_u8) {
    auto f = view_f32(field, "field");
    auto mm = view_f32(minmax, "minmax"), l = view_f32(lut, "lut");
    TORCH_CHECK(want_float || want_u8, "view_palette: no output asked for");
    TORCH_CHECK(mm.numel() == 2 && l.dim() == 2 && l.size(1) == 3, "view_palette: minmax (2) and lut (L,3) expected");
    TORCH_CHECK(mm.device() == f.device() && l.device() == f.device(), "view_palette: minmax and lut must live on the field's device");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(f.device());
    const long long HW = f.numel();
    c10::optional<torch::Tensor> of, ou;
    std::vector<int64_t> sf{3}, su(f.sizes().begin(), f.sizes().end());
    sf.insert(sf.end(), f.sizes().begin(), f.sizes().end());
    su.push_back(3);
    if (want_float) of = torch::empty(sf, f.options());
    if (want_u8) ou = torch::empty(su, f.options().dtype(torch::kUInt8));
    check_status(f3dgs_view_palette(HW, fptr(f), mm.data_ptr<float>(), l.data_ptr<float>(), (int)std::min<int64_t>(l.size(0), 1 << 20),
                                    (int)mode, (want_float && HW) ? of->data_ptr<float>() : nullptr,
                                    (want_u8 && HW) ? ou->data_ptr<uint8_t>() : nullptr, current_stream(f)),
                 "view_palette");
    return std::make_tuple(of, ou);
}

// image (3,H,W) float32 -> (H,W,3) uint8: clamp(c, 0, 1) * 255, truncated
torch::Tensor ViewBytes(const torch::Tensor& image) {
    auto im = view_f32(image, "image");
    TORCH_CHECK(im.dim() == 3 && im.size(0) == 3, "view_bytes: image (3,H,W) expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(im.device());
    torch::Tensor out = torch::empty({im.size(1), im.size(2), 3}, im.options().dtype(torch::kUInt8));
    const long long HW = im.size(1) * im.size(2);
    check_status(f3dgs_view_bytes(HW, fptr(im), HW ? out.data_ptr<uint8_t>() : nullptr, current_stream(im)), "view_bytes");
    return out;
}

// One byte per row, non-zero where the mask is: bool / uint8 masks as they are, wider types through `!= 0` (a cast to
// uint8 would wrap: an int32 `radii` of 256 handed in as the mask would read as "not visible").
static torch::Tensor mask_bytes(const torch::Tensor& row_mask) {
    if (row_mask.scalar_type() == torch::kBool || row_mask.scalar_type() == torch::kUInt8) return row_mask.contiguous();
    return row_mask.ne(0);
}

void AdamStep(torch::Tensor& param, const torch::Tensor& grad, torch::Tensor& exp_avg, torch::Tensor& exp_avg_sq, double lr,
              double beta1, double beta2, double eps, int64_t step, const c10::optional<torch::Tensor>& row_mask) {
    TORCH_CHECK(param.is_cuda() && grad.is_cuda() && exp_avg.is_cuda() && exp_avg_sq.is_cuda(), "adam_step: HIP tensors only");
    TORCH_CHECK(param.scalar_type() == torch::kFloat32 && grad.scalar_type() == torch::kFloat32, "adam_step: float32 only");
    TORCH_CHECK(param.is_contiguous() && exp_avg.is_contiguous() && exp_avg_sq.is_contiguous(), "adam_step: contiguous state");
    TORCH_CHECK(grad.numel() == param.numel() && exp_avg.numel() == param.numel() && exp_avg_sq.numel() == param.numel(),
                "adam_step: size mismatch");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(param.device());
    auto g = grad.contiguous();
    const uint8_t* mask = nullptr;
    size_t width = 1;
    torch::Tensor mk;
    if (row_mask.has_value() && row_mask->defined()) {
        TORCH_CHECK(param.dim() >= 1 && row_mask->numel() == param.size(0), "adam_step: one mask entry per row");
        TORCH_CHECK(row_mask->is_cuda(), "adam_step: the mask must be a HIP tensor");
        mk = mask_bytes(*row_mask);
        mask = static_cast<const uint8_t*>(mk.data_ptr());
        width = param.size(0) ? (size_t)(param.numel() / param.size(0)) : 1;
    }
    check_status(f3dgs_adam_step_rows((size_t)param.numel(), width, mask, param.data_ptr<float>(), g.data_ptr<float>(),
                                      exp_avg.data_ptr<float>(), exp_avg_sq.data_ptr<float>(), lr, beta1, beta2, eps, (int)step,
                                      current_stream(param)),
                 "adam_step");
}

// torch.optim.Adam's step over a list of tensors in one launch (include/f3dgs.h: f3dgs_adam_step_multi).
void AdamStepMulti(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads, std::vector<torch::Tensor> exp_avgs,
                   std::vector<torch::Tensor> exp_avg_sqs, std::vector<double> lrs, double beta1, double beta2, double eps,
                   std::vector<int64_t> steps, const c10::optional<torch::Tensor>& row_mask) {
    const size_t n = params.size();
    TORCH_CHECK(n <= F3DGS_ADAM_MAX_TENSORS, "adam_step_multi: at most ", F3DGS_ADAM_MAX_TENSORS, " tensors per call");
    TORCH_CHECK(grads.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n && lrs.size() == n && steps.size() == n,
                "adam_step_multi: list lengths differ");
    if (n == 0) return;
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params[0].device());
    std::vector<torch::Tensor> keep;       // contiguous copies of gradients stay alive until the launch is enqueued
    f3dgs_adam_tensor tab[F3DGS_ADAM_MAX_TENSORS];
    for (size_t i = 0; i < n; i++) {
        TORCH_CHECK(params[i].is_cuda() && grads[i].is_cuda() && exp_avgs[i].is_cuda() && exp_avg_sqs[i].is_cuda(), "adam_step_multi: HIP tensors only");
        TORCH_CHECK(params[i].scalar_type() == torch::kFloat32 && grads[i].scalar_type() == torch::kFloat32, "adam_step_multi: float32 only");
        TORCH_CHECK(params[i].is_contiguous() && exp_avgs[i].is_contiguous() && exp_avg_sqs[i].is_contiguous(), "adam_step_multi: contiguous state");
        TORCH_CHECK(grads[i].numel() == params[i].numel() && exp_avgs[i].numel() == params[i].numel() &&
                    exp_avg_sqs[i].numel() == params[i].numel(), "adam_step_multi: size mismatch");
        keep.push_back(grads[i].contiguous());
        tab[i] = f3dgs_adam_tensor{params[i].data_ptr<float>(), keep.back().data_ptr<float>(), exp_avgs[i].data_ptr<float>(),
                                   exp_avg_sqs[i].data_ptr<float>(), (size_t)params[i].numel(), lrs[i], (int)steps[i]};
    }
    const uint8_t* mask = nullptr;
    size_t rows = 0;
    torch::Tensor mk;
    if (row_mask.has_value() && row_mask->defined()) {
        TORCH_CHECK(row_mask->is_cuda(), "adam_step_multi: the mask must be a HIP tensor");
        mk = mask_bytes(*row_mask);
        mask = static_cast<const uint8_t*>(mk.data_ptr());
        rows = (size_t)mk.numel();
    }
    check_status(f3dgs_adam_step_multi((int)n, tab, beta1, beta2, eps, mask, rows, current_stream(params[0])), "adam_step_multi");
}

// The capturable step (include/f3dgs.h: f3dgs_adam_schedule + f3dgs_adam_step_multi_device): step counts, rates and the two
// constants live on the device.  steps[i]: float32 scalar; lr_table: float64, tensor i's base rate at lr_slots[i];
// schedules[i]: empty, or {lr_init, lr_final, lr_delay_steps, lr_delay_mult, max_steps}; iteration: int64 scalar (or None);
// consts: float64 (F3DGS_ADAM_MAX_TENSORS, 2) - column 0 is the rate used, column 1 holds the two fp32 constants.
// `phases`: 1 the schedule launch only, 2 the step launch only, 3 both.
void AdamStepMultiDevice(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads, std::vector<torch::Tensor> exp_avgs,
                         std::vector<torch::Tensor> exp_avg_sqs, std::vector<torch::Tensor> steps, const torch::Tensor& lr_table,
                         std::vector<int64_t> lr_slots, std::vector<std::vector<double>> schedules, double beta1, double beta2,
                         double eps, const c10::optional<torch::Tensor>& iteration, bool advance, torch::Tensor& consts,
                         const c10::optional<torch::Tensor>& row_mask, int64_t phases) {
    const char* who = "adam_step_multi_device";
    const size_t n = params.size();
    TORCH_CHECK(n <= F3DGS_ADAM_MAX_TENSORS, who, ": at most ", F3DGS_ADAM_MAX_TENSORS, " tensors per call");
    TORCH_CHECK(grads.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n && steps.size() == n && lr_slots.size() == n &&
                schedules.size() == n, who, ": list lengths differ");
    if (n == 0) return;
    TORCH_CHECK(lr_table.is_cuda() && lr_table.scalar_type() == torch::kFloat64 && lr_table.is_contiguous(), who, ": lr_table must be a contiguous float64 HIP tensor");
    TORCH_CHECK(consts.is_cuda() && consts.scalar_type() == torch::kFloat64 && consts.is_contiguous() &&
                consts.numel() == 2 * F3DGS_ADAM_MAX_TENSORS, who, ": consts must be a contiguous float64 HIP tensor of ", 2 * F3DGS_ADAM_MAX_TENSORS, " elements");
    static_assert(sizeof(f3dgs_adam_consts) == 2 * sizeof(double), "consts layout");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params[0].device());
    std::vector<torch::Tensor> keep;       // contiguous copies of gradients stay alive until the launch is enqueued
    f3dgs_adam_device_tensor tab[F3DGS_ADAM_MAX_TENSORS];
    for (size_t i = 0; i < n; i++) {
        TORCH_CHECK(params[i].is_cuda() && grads[i].is_cuda() && exp_avgs[i].is_cuda() && exp_avg_sqs[i].is_cuda() && steps[i].is_cuda(), who, ": HIP tensors only");
        TORCH_CHECK(params[i].scalar_type() == torch::kFloat32 && grads[i].scalar_type() == torch::kFloat32, who, ": float32 only");
        TORCH_CHECK(steps[i].scalar_type() == torch::kFloat32 && steps[i].numel() == 1, who, ": the step word is one float32");
        TORCH_CHECK(params[i].is_contiguous() && exp_avgs[i].is_contiguous() && exp_avg_sqs[i].is_contiguous(), who, ": contiguous state");
        TORCH_CHECK(grads[i].numel() == params[i].numel() && exp_avgs[i].numel() == params[i].numel() &&
                    exp_avg_sqs[i].numel() == params[i].numel(), who, ": size mismatch");
        TORCH_CHECK(lr_slots[i] >= 0 && lr_slots[i] < lr_table.numel(), who, ": lr slot outside the table");
        TORCH_CHECK(schedules[i].empty() || schedules[i].size() == 5, who, ": a schedule is (lr_init, lr_final, lr_delay_steps, lr_delay_mult, max_steps)");
        keep.push_back(grads[i].contiguous());
        f3dgs_adam_device_tensor& t = tab[i];
        t = f3dgs_adam_device_tensor{};
        t.param = params[i].data_ptr<float>(); t.grad = keep.back().data_ptr<float>();
        t.exp_avg = exp_avgs[i].data_ptr<float>(); t.exp_avg_sq = exp_avg_sqs[i].data_ptr<float>();
        t.n = (size_t)params[i].numel();
        t.step = steps[i].data_ptr<float>();
        t.lr = lr_table.data_ptr<double>() + lr_slots[i];
        if (!schedules[i].empty()) {
            const auto& sc = schedules[i];
            t.scheduled = 1;
            t.lr_init = sc[0]; t.lr_final = sc[1]; t.lr_delay_steps = (long long)sc[2]; t.lr_delay_mult = sc[3]; t.max_steps = (long long)sc[4];
        }
    }
    long long* it = nullptr;
    if (iteration.has_value() && iteration->defined()) {
        TORCH_CHECK(iteration->is_cuda() && iteration->scalar_type() == torch::kInt64 && iteration->numel() == 1, who, ": the iteration word is one int64 on the device");
        it = reinterpret_cast<long long*>(iteration->data_ptr<int64_t>());
    }
    const uint8_t* mask = nullptr;
    size_t rows = 0;
    torch::Tensor mk;
    if (row_mask.has_value() && row_mask->defined()) {
        TORCH_CHECK(row_mask->is_cuda(), who, ": the mask must be a HIP tensor");
        mk = mask_bytes(*row_mask);
        mask = static_cast<const uint8_t*>(mk.data_ptr());
        rows = (size_t)mk.numel();
    }
    auto* cs = reinterpret_cast<f3dgs_adam_consts*>(consts.data_ptr<double>());
    if (phases & 1) check_status(f3dgs_adam_schedule((int)n, tab, beta1, beta2, it, advance ? 1 : 0, cs, current_stream(params[0])), who);
    if (phases & 2) check_status(f3dgs_adam_step_multi_device((int)n, tab, beta1, beta2, eps, mask, rows, cs, current_stream(params[0])), who);
}

// The reference's reset_opacity in place (include/f3dgs.h: f3dgs_reset_opacity); the moments may be None.
void ResetOpacity(torch::Tensor& raw, const c10::optional<torch::Tensor>& exp_avg, const c10::optional<torch::Tensor>& exp_avg_sq, double cap) {
    TORCH_CHECK(raw.is_cuda() && raw.scalar_type() == torch::kFloat32 && raw.is_contiguous(), "reset_opacity: a contiguous float32 HIP tensor expected");
    float* mv[2] = {nullptr, nullptr};
    const c10::optional<torch::Tensor>* in[2] = {&exp_avg, &exp_avg_sq};
    for (int k = 0; k < 2; k++) {
        if (!in[k]->has_value() || !(*in[k])->defined()) continue;
        const torch::Tensor& t = **in[k];
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.numel() == raw.numel(), "reset_opacity: the moments must match the parameter");
        mv[k] = t.numel() ? t.data_ptr<float>() : nullptr;
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(raw.device());
    check_status(f3dgs_reset_opacity((size_t)raw.numel(), raw.numel() ? raw.data_ptr<float>() : nullptr, mv[0], mv[1], (float)cap, current_stream(raw)),
                 "reset_opacity");
}

// One gather over all per-Gaussian tensors (densify.py builds the plan).  `modes[i]`: F3DGS_DENSIFY_*;
// `overrides[i]` is the child-row array for mode OVERRIDE_CHILD (an empty tensor otherwise).
void DensifyGather(const torch::Tensor& src_row, const torch::Tensor& kind, const torch::Tensor& override_row,
                   const std::vector<torch::Tensor>& srcs, std::vector<torch::Tensor>& dsts,
                   const std::vector<torch::Tensor>& overrides, const std::vector<int64_t>& modes) {
    const size_t n_out = (size_t)src_row.numel();
    TORCH_CHECK(src_row.is_cuda() && src_row.scalar_type() == torch::kInt32 && src_row.is_contiguous(), "densify_gather: src_row must be a contiguous int32 HIP tensor");
    TORCH_CHECK(kind.is_cuda() && kind.scalar_type() == torch::kUInt8 && kind.is_contiguous() && (size_t)kind.numel() == n_out, "densify_gather: kind must be uint8 of the same length");
    TORCH_CHECK(override_row.is_cuda() && override_row.scalar_type() == torch::kInt32 && override_row.is_contiguous() && (size_t)override_row.numel() == n_out,
                "densify_gather: override_row must be int32 of the same length");
    TORCH_CHECK(srcs.size() == dsts.size() && srcs.size() == modes.size() && srcs.size() == overrides.size(), "densify_gather: list lengths differ");
    std::vector<f3dgs_densify_tensor> table(srcs.size());
    for (size_t i = 0; i < srcs.size(); i++) {
        const auto& a = srcs[i];
        auto& d = dsts[i];
        TORCH_CHECK(a.is_cuda() && d.is_cuda() && a.scalar_type() == torch::kFloat32 && d.scalar_type() == torch::kFloat32, "densify_gather: float32 HIP tensors only");
        TORCH_CHECK(a.is_contiguous() && d.is_contiguous(), "densify_gather: contiguous tensors only");
        int64_t width = 1;
        for (int64_t k = 1; k < a.dim(); k++) width *= a.size(k);
        TORCH_CHECK(a.dim() >= 1 && width >= 1, "densify_gather: tensors are (rows, ...) with non-empty rows");
        TORCH_CHECK((size_t)d.numel() >= n_out * (size_t)width, "densify_gather: destination ", i, " too small");
        table[i].src = a.data_ptr<float>();
        table[i].dst = d.data_ptr<float>();
        table[i].width = (int)width;
        table[i].mode = (int)modes[i];
        table[i].override_src = nullptr;
        if (modes[i] == F3DGS_DENSIFY_OVERRIDE_CHILD) {
            const auto& o = overrides[i];
            TORCH_CHECK(o.is_cuda() && o.scalar_type() == torch::kFloat32 && o.is_contiguous(), "densify_gather: override must be a contiguous float32 HIP tensor");
            table[i].override_src = o.numel() ? o.data_ptr<float>() : a.data_ptr<float>();   // no children: never read
        }
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(src_row.device());
    check_status(f3dgs_densify_gather(n_out, src_row.data_ptr<int32_t>(), kind.data_ptr<uint8_t>(), override_row.data_ptr<int32_t>(),
                                      (int)table.size(), table.data(), current_stream(src_row)),
                 "densify_gather");
}

// The model's front end (include/f3dgs.h: f3dgs_activate_forward / _backward, f3dgs_densify_stats; model_front.py).  An input
// is `None` or a float32 HIP tensor; a non-contiguous view is copied, and so is a misaligned one where the library reads
// with 16-byte loads (dev_f32).
using OptT = c10::optional<torch::Tensor>;

static bool given(const OptT& t) { return t.has_value() && t->defined(); }

static torch::Tensor front_in(const OptT& t, const char* name, int64_t P, int64_t per_row, bool align16) {
    if (!given(t)) return torch::Tensor();
    TORCH_CHECK(t->is_cuda(), name, " must live on a HIP device (got ", t->device(), "): the model front end has no CPU path");
    TORCH_CHECK(t->scalar_type() == torch::kFloat32, name, " must be float32");
    TORCH_CHECK(t->numel() == P * per_row, name, ": ", P * per_row, " elements expected, got ", t->sizes());
    torch::Tensor c = t->contiguous();
    if (align16 && c.numel() && (reinterpret_cast<uintptr_t>(c.data_ptr()) & 15)) c = c.clone();
    return c;
}

static const float* cptr(const torch::Tensor& t) { return t.defined() && t.numel() ? t.data_ptr<float>() : nullptr; }
static float* mptr(torch::Tensor& t) { return t.defined() && t.numel() ? t.data_ptr<float>() : nullptr; }
static OptT opt_out(const torch::Tensor& t) { return t.defined() ? OptT(t) : OptT(); }

std::tuple<OptT, OptT, OptT, OptT> ActivateForward(const OptT& scaling, const OptT& rotation, const OptT& opacity, const OptT& features_dc,
                                                   const OptT& features_rest) {
    const OptT* first = nullptr;
    for (const OptT* t : {&scaling, &rotation, &opacity, &features_dc})
        if (given(*t)) { first = t; break; }
    TORCH_CHECK(first, "activate_forward: every group is None");
    TORCH_CHECK(given(features_dc) || !given(features_rest), "activate_forward: features_rest without features_dc");
    TORCH_CHECK((*first)->dim() >= 1, "activate_forward: tensors are (P, ...)");
    const int64_t P = (*first)->size(0);
    int64_t M = 1;
    if (given(features_rest)) {
        TORCH_CHECK(features_rest->dim() == 3 && features_rest->size(0) == P && features_rest->size(2) == 3,
                    "activate_forward: features_rest must be (P, M - 1, 3); got ", features_rest->sizes());
        M = 1 + features_rest->size(1);
    }
    auto sc = front_in(scaling, "scaling", P, 3, false), rot = front_in(rotation, "rotation", P, 4, false),
         op = front_in(opacity, "opacity", P, 1, false), dc = front_in(features_dc, "features_dc", P, 3, false),
         rest = front_in(features_rest, "features_rest", P, 3 * (M - 1), false);
    c10::hip::HIPGuardMasqueradingAsCUDA guard((*first)->device());
    torch::Tensor scales, rotations, opacities, shs;
    if (sc.defined()) scales = torch::empty({P, 3}, sc.options());
    if (rot.defined()) rotations = torch::empty({P, 4}, rot.options());
    if (op.defined()) opacities = torch::empty(opacity->sizes(), op.options());
    if (dc.defined()) shs = torch::empty({P, M, 3}, dc.options());
    check_status(f3dgs_activate_forward((int)P, (int)M, cptr(sc), cptr(rot), cptr(op), cptr(dc), cptr(rest), mptr(scales), mptr(rotations),
                                        mptr(opacities), mptr(shs), current_stream(**first)),
                 "activate_forward");
    return std::make_tuple(opt_out(scales), opt_out(rotations), opt_out(opacities), opt_out(shs));
}

// `want`: which of (d_scaling, d_rotation, d_opacity, d_features_dc, d_features_rest) to produce; the others come back None.
// scales / opacities: the forward's outputs, raw_rotation: its input; an upstream gradient that is None counts as zeros.
std::tuple<OptT, OptT, OptT, OptT, OptT> ActivateBackward(int64_t P, int64_t M, const OptT& scales, const OptT& raw_rotation,
                                                          const OptT& opacities, const OptT& dL_dscale, const OptT& dL_drot,
                                                          const OptT& dL_dopacity, const OptT& dL_dsh, std::array<bool, 5> want,
                                                          const torch::Tensor& like) {
    TORCH_CHECK(like.is_cuda(), "activate_backward: HIP tensors only");
    TORCH_CHECK(P >= 0 && M >= 1, "activate_backward: bad sizes");
    auto sc = front_in(scales, "scales", P, 3, false), rot = front_in(raw_rotation, "raw_rotation", P, 4, false),
         op = front_in(opacities, "opacities", P, 1, false), gs = front_in(dL_dscale, "dL_dscale", P, 3, false),
         gr = front_in(dL_drot, "dL_drot", P, 4, false), go = front_in(dL_dopacity, "dL_dopacity", P, 1, false),
         gsh = front_in(dL_dsh, "dL_dsh", P, 3 * M, true);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(like.device());
    auto f32 = like.options().dtype(torch::kFloat32);
    torch::Tensor ds, dr, dop, ddc, drest;
    if (want[0]) ds = torch::empty({P, 3}, f32);
    if (want[1]) dr = torch::empty({P, 4}, f32);
    if (want[2]) dop = op.defined() ? torch::empty(op.sizes(), f32) : torch::empty({P, 1}, f32);
    if (want[3]) ddc = torch::empty({P, 1, 3}, f32);
    if (want[4]) drest = torch::empty({P, M - 1, 3}, f32);
    check_status(f3dgs_activate_backward((int)P, (int)M, cptr(sc), cptr(rot), cptr(op), cptr(gs), cptr(gr), cptr(go), cptr(gsh), mptr(ds),
                                         mptr(dr), mptr(dop), mptr(ddc), mptr(drest), current_stream(like)),
                 "activate_backward");
    return std::make_tuple(opt_out(ds), opt_out(dr), opt_out(dop), opt_out(ddc), opt_out(drest));
}

// In place on the three accumulators (each None or a contiguous float32 HIP tensor of P elements).
void DensifyStats(const OptT& viewspace_grad, const torch::Tensor& radii, OptT xyz_gradient_accum, OptT denom, OptT max_radii2D) {
    TORCH_CHECK(radii.is_cuda(), "densify_stats: radii must live on a HIP device");
    const int64_t P = radii.numel();
    torch::Tensor r = radii.scalar_type() == torch::kInt32 ? radii.contiguous() : radii.to(torch::kInt32).contiguous();
    torch::Tensor g = front_in(viewspace_grad, "viewspace_grad", P, 3, false);
    float* acc[3] = {nullptr, nullptr, nullptr};
    const OptT* in[3] = {&xyz_gradient_accum, &denom, &max_radii2D};
    const char* names[3] = {"xyz_gradient_accum", "denom", "max_radii2D"};
    for (int k = 0; k < 3; k++) {
        if (!given(*in[k])) continue;
        const torch::Tensor& t = **in[k];
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.numel() == P, "densify_stats: ", names[k],
                    " must be a contiguous float32 HIP tensor of ", P, " elements (it is updated in place)");
        acc[k] = P ? t.data_ptr<float>() : nullptr;
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(radii.device());
    check_status(f3dgs_densify_stats((int)P, cptr(g), P ? r.data_ptr<int32_t>() : nullptr, acc[0], acc[1], acc[2], current_stream(radii)),
                 "densify_stats");
}

}  // namespace

PYBIND11_MODULE(_C, m) {
    m.def("rasterize_gaussians", &RasterizeGaussians);
    m.def("rasterize_gaussians_backward", &RasterizeGaussiansBackward);
    m.def("mark_visible", &markVisible);
    m.def("feature_l1", &FeatureL1, py::arg("feature_map"), py::arg("gt"), py::arg("weight"), py::arg("bias"), py::arg("dense") = true);
    m.def("set_feature_grad_lowres", [](py::object gx, py::object scale) {
              auto& h = feature_grad_lowres();
              h.first = gx.is_none() ? torch::Tensor() : gx.cast<torch::Tensor>();
              h.second = (gx.is_none() || scale.is_none()) ? torch::Tensor() : scale.cast<torch::Tensor>();
          },
          py::arg("gx"), py::arg("scale") = py::none(),
          "gx (Hg, Wg, C) float32 = dL/d(resized feature map) as feature_l1 returns it, scale = 0-dim device tensor or None: the NEXT "
          "rasterize_gaussians_backward call takes its feature-map gradient from there (transposed resize applied per tile); None clears");
    m.def("feature_decode", &FeatureDecode);
    m.def("image_loss_forward", &ImageLossForward, py::arg("image"), py::arg("gt"), py::arg("lambda_dssim"), py::arg("want_grad"),
          py::arg("per_image") = false);
    m.def("image_loss_backward", &ImageLossBackward, py::arg("image"), py::arg("gt"), py::arg("scratch"), py::arg("upstream"),
          py::arg("lambda_dssim"), py::arg("mode"));
    m.attr("IMAGE_LOSS_L1_DSSIM") = (int)F3DGS_IMAGE_LOSS_L1_DSSIM;
    m.attr("IMAGE_LOSS_SSIM") = (int)F3DGS_IMAGE_LOSS_SSIM;
    m.attr("IMAGE_LOSS_SSIM_PER_IMAGE") = (int)F3DGS_IMAGE_LOSS_SSIM_PER_IMAGE;
    m.def("image_metrics", &ImageMetrics, py::arg("image"), py::arg("gt"), py::arg("image_format"), py::arg("gt_format"), py::arg("flags"),
          py::arg("want_ssim") = true);
    m.attr("IMAGE_F32") = (int)F3DGS_IMAGE_F32;
    m.attr("IMAGE_U8_PLANAR") = (int)F3DGS_IMAGE_U8_PLANAR;
    m.attr("IMAGE_U8_INTERLEAVED") = (int)F3DGS_IMAGE_U8_INTERLEAVED;
    m.attr("METRICS_QUANTIZE_IMAGE") = (int)F3DGS_METRICS_QUANTIZE_IMAGE;
    m.attr("METRICS_QUANTIZE_GT") = (int)F3DGS_METRICS_QUANTIZE_GT;
    m.def("edit_select", &EditSelect, py::arg("features"), py::arg("text"), py::arg("positive_mask"), py::arg("first_positive"),
          py::arg("variant"), py::arg("threshold") = py::none(), py::arg("normalize_inplace") = false, py::arg("want_score") = false,
          py::arg("opacity") = py::none());
    m.def("segment", &Segment, py::arg("feature_map"), py::arg("text"), py::arg("Hs"), py::arg("Ws"), py::arg("weight"), py::arg("bias"),
          py::arg("flags"), py::arg("want_score"));
    m.def("contributions", &Contributions, py::arg("geomBuffer"), py::arg("binningBuffer"), py::arg("imgBuffer"), py::arg("P"),
          py::arg("num_rendered"), py::arg("H"), py::arg("W"), py::arg("masks") = py::none(), py::arg("acc") = py::none(),
          py::arg("wmax") = py::none(), py::arg("want_pixel") = true);
    m.attr("CONTRIB_MAX_MASKS") = (int)F3DGS_CONTRIB_MAX_MASKS;
    m.def("label_votes", &LabelVotes, py::arg("geomBuffer"), py::arg("binningBuffer"), py::arg("imgBuffer"), py::arg("P"),
          py::arg("num_rendered"), py::arg("H"), py::arg("W"), py::arg("labels"), py::arg("L"), py::arg("acc"));
    m.attr("LABEL_VOTES_MAX_LABELS") = (int)F3DGS_LABEL_VOTES_MAX_LABELS;
    m.def("instance_associate", &InstanceAssociate, py::arg("acc_view"), py::arg("acc"), py::arg("count"), py::arg("dropped"),
          py::arg("iou_thresh"), py::arg("min_weight"));
    m.def("instance_merge", &InstanceMerge, py::arg("acc_view"), py::arg("mapping"), py::arg("acc"), py::arg("clear_view"));
    m.attr("INSTANCE_MAX_MASKS") = (int)F3DGS_INSTANCE_MAX_MASKS;
    m.attr("INSTANCE_MAX_INSTANCES") = (int)F3DGS_INSTANCE_MAX_INSTANCES;
    m.def("feature_pca_moments", &FeaturePcaMoments, py::arg("feature_map"), py::arg("stride"));
    m.def("feature_pca_project", &FeaturePcaProject, py::arg("feature_map"), py::arg("mean"), py::arg("components"),
          py::arg("lo") = py::none(), py::arg("hi") = py::none());
    m.attr("FEATURE_PCA_MAX_CHANNELS") = (int)F3DGS_FEATURE_PCA_MAX_CHANNELS;
    m.def("view_normals", &ViewNormals, py::arg("depth"), py::arg("projection_matrix"), py::arg("inv_full_proj"), py::arg("chw") = false,
          py::arg("half") = false);
    m.def("view_gradient", &ViewGradient, py::arg("image"));
    m.def("view_curvature", &ViewCurvature, py::arg("depth"), py::arg("projection_matrix"), py::arg("inv_full_proj"));
    m.def("view_minmax", &ViewMinmax, py::arg("field"));
    m.def("view_palette", &ViewPalette, py::arg("field"), py::arg("minmax"), py::arg("lut"), py::arg("mode"), py::arg("want_float") = true,
          py::arg("want_u8") = false);
    m.def("view_bytes", &ViewBytes, py::arg("image"));
    m.attr("VIEW_TILE") = (int)F3DGS_VIEW_TILE;
    m.attr("VIEW_PALETTE_MINMAX") = (int)F3DGS_VIEW_PALETTE_MINMAX;
    m.attr("VIEW_PALETTE_MAX") = (int)F3DGS_VIEW_PALETTE_MAX;
    m.attr("VIEW_PALETTE_MAX_ENTRIES") = (int)F3DGS_VIEW_PALETTE_MAX_ENTRIES;
    m.attr("SEGMENT_ROUND_HALF") = (int)F3DGS_SEGMENT_ROUND_HALF;
    m.attr("SEGMENT_TEXT_NORMALIZED") = (int)F3DGS_SEGMENT_TEXT_NORMALIZED;
    m.attr("SEGMENT_MAX_TEXTS") = (int)F3DGS_SEGMENT_MAX_TEXTS;
    m.def("seg_metrics", &SegMetrics, py::arg("teacher"), py::arg("student"), py::arg("gt"), py::arg("num_labels"), py::arg("num_classes"),
          py::arg("carry_counts"), py::arg("carry_scalars"), py::arg("want_scores"));
    m.def("seg_colorize", &SegColorize, py::arg("labels"), py::arg("palette"), py::arg("image"), py::arg("mode"), py::arg("a"), py::arg("b"),
          py::arg("fill"));
    m.def("sam_masks", &SamMasks, py::arg("low_res"), py::arg("iou_preds"), py::arg("pred_iou_thresh"), py::arg("S"), py::arg("ih"),
          py::arg("iw"), py::arg("H"), py::arg("W"), py::arg("FH"), py::arg("FW"), py::arg("cx0"), py::arg("cy0"), py::arg("t"), py::arg("t_hi"),
          py::arg("t_lo"), py::arg("stability_thresh"), py::arg("edge_filter"));
    m.def("sam_upscale", &SamUpscale, py::arg("low_res"), py::arg("S"), py::arg("ih"), py::arg("iw"), py::arg("H"), py::arg("W"), py::arg("t"),
          py::arg("out_bool"));
    m.def("sam_decoder_pack", &SamDecoderPack, py::arg("params"));
    m.def("sam_decoder_plan", &SamDecoderPlan, py::arg("packed"), py::arg("features"));
    m.def("sam_decoder_predict", &SamDecoderPredict, py::arg("plan"), py::arg("packed"), py::arg("h"), py::arg("w"), py::arg("coords"),
          py::arg("labels"), py::arg("boxes"), py::arg("input_h"), py::arg("input_w"), py::arg("multimask"));
    m.def("lpips_pack", &LpipsPack, py::arg("params"));
    m.def("lpips_workspace_bytes", &LpipsWorkspaceBytes, py::arg("N"), py::arg("H"), py::arg("W"));
    m.def("lpips_forward", &LpipsForward, py::arg("packed"), py::arg("x"), py::arg("y"), py::arg("flags"));
    m.def("lpips_taps", &LpipsTaps, py::arg("packed"), py::arg("image"), py::arg("quantize"));
    m.attr("LPIPS_QUANTIZE_X") = (int)F3DGS_LPIPS_QUANTIZE_X;
    m.attr("LPIPS_QUANTIZE_Y") = (int)F3DGS_LPIPS_QUANTIZE_Y;
    m.def("box_nms", &BoxNms, py::arg("boxes"), py::arg("categories"), py::arg("iou_threshold"), py::arg("order"));
    m.def("mask_rle_count", &MaskRleCount, py::arg("packed"), py::arg("index"), py::arg("FH"));
    m.def("mask_rle_emit", &MaskRleEmit, py::arg("packed"), py::arg("index"), py::arg("FH"), py::arg("lens"), py::arg("ends"), py::arg("out"),
          py::arg("head"));
    m.def("mask_unpack", &MaskUnpack, py::arg("packed"), py::arg("index"), py::arg("FH"));
    m.def("mask_instance_map", &MaskInstanceMap, py::arg("packed"), py::arg("index"), py::arg("FH"));
    m.def("mask_regions", &MaskRegions, py::arg("packed"), py::arg("index"), py::arg("FH"), py::arg("area_thresh"), py::arg("holes"),
          py::arg("run_capacity"));
    m.attr("BOX_NMS_MAX") = (int)F3DGS_BOX_NMS_MAX;
    m.attr("LABELS_U8") = (int)F3DGS_LABELS_U8;
    m.attr("LABELS_I32") = (int)F3DGS_LABELS_I32;
    m.attr("LABELS_I64") = (int)F3DGS_LABELS_I64;
    m.attr("SEG_COLOR_MASK") = (int)F3DGS_SEG_COLOR_MASK;
    m.attr("SEG_COLOR_BLEND") = (int)F3DGS_SEG_COLOR_BLEND;
    m.attr("SEG_COLOR_STRIP") = (int)F3DGS_SEG_COLOR_STRIP;
    m.attr("EDIT_SELECT") = (int)F3DGS_EDIT_SELECT;
    m.attr("EDIT_DELETE") = (int)F3DGS_EDIT_DELETE;
    m.attr("EDIT_TEXT_NORMALIZED") = (int)F3DGS_EDIT_TEXT_NORMALIZED;
    m.attr("EDIT_FILL_UNSELECTED") = (int)F3DGS_EDIT_FILL_UNSELECTED;
    m.attr("EDIT_MAX_TEXTS") = (int)F3DGS_EDIT_MAX_TEXTS;
    m.attr("EDIT_MAX_TEXT_ELEMENTS") = (int)F3DGS_EDIT_MAX_TEXT_ELEMENTS;
    m.def("adam_step", &AdamStep, py::arg("param"), py::arg("grad"), py::arg("exp_avg"), py::arg("exp_avg_sq"), py::arg("lr"),
          py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("step"), py::arg("row_mask") = py::none());
    m.def("adam_step_multi", &AdamStepMulti, py::arg("params"), py::arg("grads"), py::arg("exp_avgs"), py::arg("exp_avg_sqs"), py::arg("lrs"),
          py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("steps"), py::arg("row_mask") = py::none());
    m.def("adam_step_multi_device", &AdamStepMultiDevice, py::arg("params"), py::arg("grads"), py::arg("exp_avgs"), py::arg("exp_avg_sqs"),
          py::arg("steps"), py::arg("lr_table"), py::arg("lr_slots"), py::arg("schedules"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
          py::arg("iteration"), py::arg("advance"), py::arg("consts"), py::arg("row_mask") = py::none(), py::arg("phases") = 3);
    m.def("reset_opacity", &ResetOpacity, py::arg("raw"), py::arg("exp_avg"), py::arg("exp_avg_sq"), py::arg("cap"));
    m.def("densify_gather", &DensifyGather);
    m.def("activate_forward", &ActivateForward, py::arg("scaling"), py::arg("rotation"), py::arg("opacity"), py::arg("features_dc"),
          py::arg("features_rest"));
    m.def("activate_backward", &ActivateBackward, py::arg("P"), py::arg("M"), py::arg("scales"), py::arg("raw_rotation"), py::arg("opacities"),
          py::arg("dL_dscale"), py::arg("dL_drot"), py::arg("dL_dopacity"), py::arg("dL_dsh"), py::arg("want"), py::arg("like"));
    m.def("densify_stats", &DensifyStats, py::arg("viewspace_grad"), py::arg("radii"), py::arg("xyz_gradient_accum"), py::arg("denom"),
          py::arg("max_radii2D"));
    m.def("version", []() { return f3dgs_version(); });
    m.def("set_feature_grad_hook", [](py::object fn) { feature_grad_hook() = std::move(fn); },
          "callable(dL_dsemantic_feature) run inside rasterize_gaussians_backward once that tensor is final on the stream; None removes it");
    m.def("set_feature_grad_accumulator", [](py::object t) {
              if (t.is_none()) feature_grad_accumulator() = torch::Tensor();
              else feature_grad_accumulator() = t.cast<torch::Tensor>();
          },
          "tensor (P*C float32, contiguous, on the op's device) that the following backward calls ADD dL/dsemantic_feature into "
          "(they then return an empty tensor for that gradient); None restores the default");
    m.def("set_grad_rows_hook", [](py::object fn, int chunks) { grad_rows_hook() = std::move(fn); grad_rows_chunks() = chunks > 0 ? chunks : 1; },
          py::arg("fn"), py::arg("chunks") = 4,
          "callable(row_begin, row_end, grads: dict) run inside rasterize_gaussians_backward after each of `chunks` row ranges of the "
          "per-Gaussian gradients is final on the stream; None removes it");
    m.def("set_option", [](const std::string& name, int value) { check_status(f3dgs_set_option(name.c_str(), value), "set_option"); });
    m.def("set_tile_band", [](int row_begin, int row_end) { f3dgs_set_tile_band(row_begin, row_end); }, py::arg("tile_row_begin"), py::arg("tile_row_end"),
          "forward calls of this thread list and blend only tile rows [begin, end) of the view (0, 0: the whole view); include/f3dgs.h");
    m.def("forward_counts", []() -> py::object {
        const uint32_t* w = f3dgs_forward_counts();
        if (!w) return py::none();
        // (volatile: kernel-written pinned words)
        const volatile uint32_t* v = w;
        return py::make_tuple((long long)v[0], (long long)v[1], (long long)v[2], (long long)v[3], (long long)v[4]);
    }, "(entries of the instance lists, the reference's num_rendered, long-axis flag, entries provided for, sticky no-room word) of the "
       "calling thread's most recent forward call - final once that frame's work has completed; None before the first call");
    m.def("depth_sort_info", []() -> py::object {
        const uint32_t* w = f3dgs_depth_sort_info();
        if (!w) return py::none();
        py::dict d;
        static const char* const names[] = {"none", "one_launch", "passes", "buckets", "lookback"};
        d["path"] = w[0] < 5 ? names[w[0]] : "?";
        d["buckets"] = (long long)w[1];
        d["capacity"] = (long long)w[2];
        d["largest"] = (long long)w[3];
        d["oversized"] = (long long)w[4];
        return d;
    }, "how the calling thread's most recent forward call sorted its Gaussians by depth: path ('one_launch', 'passes', 'buckets', "
       "'lookback', 'none'), and of the bucket path the bins in use, the in-LDS capacity of a bucket, the frame's largest bucket and "
       "its buckets above the capacity (the last two final once the frame's work has completed); None before the first call");
    m.def("forward_counts_address", []() { return (uintptr_t)f3dgs_forward_counts(); },
          "host address of the five uint32 words of forward_counts() (0 before the first call): a captured step keeps it and reads the words after a replay");
    m.def("clear_forward_overflow", [](uintptr_t address) { if (address) reinterpret_cast<volatile uint32_t*>(address)[4] = 0u; },
          "clears the sticky no-room word behind an address returned by forward_counts_address()");
    m.def("last_backward_contraction", []() { return f3dgs_last_backward_contraction(); },
          "1: the last blend backward of this process contracted on bf16 matrix instructions (two-term operands); 0: exact fp32; -1: none yet");
    m.def("get_option", [](const std::string& name) {
        int v = 0;
        check_status(f3dgs_get_option(name.c_str(), &v), "get_option");
        return v;
    });
    m.def("profile_reset", []() { f3dgs_profile_reset(); });
    m.def("profile_read", []() {
        const char* names[64];
        double ms[64];
        long calls[64];
        const int n = f3dgs_profile_read(names, ms, calls, 64);
        std::vector<std::tuple<std::string, double, long>> out;
        for (int i = 0; i < n; i++) out.emplace_back(names[i], ms[i], calls[i]);
        return out;
    });
}
