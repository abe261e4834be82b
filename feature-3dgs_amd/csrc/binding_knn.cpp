// binding_knn.cpp - `simple_knn._C`: the reference's second native module (submodules/simple-knn/ext.cpp:15-17,
// spatial.cu:15-25) on top of the C ABI of libf3dgs_hip.so (include/f3dgs.h: f3dgs_knn_mean_dist2).
//   distCUDA2(points (P,3) float32 on the GPU) -> (P,) float32: mean squared distance to the 3 nearest neighbours.
// Beside it, with no counterpart in the reference (neighbors.py is their Python surface):
//   knn_neighbors(points, K, want_dist2) -> (idx (P,K) int32, dist2 (P,K) float32 or None): f3dgs_knn_neighbors
//   label_mode_filter(labels, weight, idx, dist2, max_dist2, fill, labels_out, share_out): one step of f3dgs_label_mode_filter
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <stdexcept>
#include <string>

#include "../../include/f3dgs.h"

namespace {

torch::Tensor distCUDA2(const torch::Tensor& points) {
    TORCH_CHECK(points.is_cuda(), "points must live on a HIP device: simple_knn has no CPU path");
    TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "points must have dimensions (num_points, 3)");
    TORCH_CHECK(points.scalar_type() == torch::kFloat32, "points must be float32");
    const int P = (int)points.size(0);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(points.device());
    auto pts = points.contiguous();
    torch::Tensor means = torch::empty({P}, points.options());
    if (P == 0) return means;
    torch::Tensor scratch = torch::empty({(long long)f3dgs_knn_scratch_bytes(P)}, points.options().dtype(torch::kByte));
    void* stream = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(points.device().index()).stream();
    const int rc = f3dgs_knn_mean_dist2(P, pts.data_ptr<float>(), means.data_ptr<float>(), scratch.data_ptr(), stream);
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("distCUDA2: ") + f3dgs_last_error());
    return means;
}

void* current_stream(const torch::Tensor& t) {
    return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

// (idx (P, K) int32, dist2 (P, K) float32 or an undefined tensor): f3dgs_knn_neighbors
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> knn_neighbors(const torch::Tensor& points, int K, bool want_dist2) {
    TORCH_CHECK(points.is_cuda(), "points must live on a HIP device: the neighbour search has no CPU path");
    TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "points must have dimensions (num_points, 3)");
    TORCH_CHECK(points.scalar_type() == torch::kFloat32, "points must be float32");
    TORCH_CHECK(K >= 1 && K <= F3DGS_KNN_MAX_NEIGHBORS, "K = ", K, ": 1 .. ", F3DGS_KNN_MAX_NEIGHBORS, " neighbours are taken");
    TORCH_CHECK(points.size(0) < (1ll << 31) / F3DGS_KNN_MAX_NEIGHBORS, "too many points");
    const int P = (int)points.size(0);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(points.device());
    auto pts = points.contiguous();
    torch::Tensor idx = torch::empty({P, K}, points.options().dtype(torch::kInt32));
    c10::optional<torch::Tensor> dist2;
    if (want_dist2) dist2 = torch::empty({P, K}, points.options());
    if (P == 0) return {idx, dist2};
    torch::Tensor scratch = torch::empty({(long long)f3dgs_knn_neighbors_scratch_bytes(P, K)}, points.options().dtype(torch::kByte));
    const int rc = f3dgs_knn_neighbors(P, K, pts.data_ptr<float>(), idx.data_ptr<int32_t>(), want_dist2 ? dist2->data_ptr<float>() : nullptr,
                                       scratch.data_ptr(), current_stream(points));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("knn_neighbors: ") + f3dgs_last_error());
    return {idx, dist2};
}

// one step of f3dgs_label_mode_filter into the caller's labels_out (and share_out)
void label_mode_filter(const torch::Tensor& labels, const c10::optional<torch::Tensor>& weight, const torch::Tensor& idx,
                       const c10::optional<torch::Tensor>& dist2, double max_dist2, bool fill, torch::Tensor& labels_out,
                       const c10::optional<torch::Tensor>& share_out) {
    TORCH_CHECK(labels.is_cuda(), "labels must live on a HIP device: the mode filter has no CPU path");
    TORCH_CHECK(labels.dim() == 1 && labels.scalar_type() == torch::kInt32 && labels.is_contiguous(), "labels: contiguous int32 (P) expected");
    const long long P = labels.size(0);
    auto same = [&](const torch::Tensor& t) { return t.device() == labels.device() && t.is_contiguous(); };
    TORCH_CHECK(idx.dim() == 2 && idx.size(0) == P && idx.scalar_type() == torch::kInt32 && same(idx),
                "idx: contiguous int32 (P, K) on the labels' device expected");
    const int K = (int)idx.size(1);
    TORCH_CHECK(labels_out.dim() == 1 && labels_out.size(0) == P && labels_out.scalar_type() == torch::kInt32 && same(labels_out),
                "labels_out: contiguous int32 (P) on the labels' device expected");
    if (weight) TORCH_CHECK(weight->dim() == 1 && weight->size(0) == P && weight->scalar_type() == torch::kFloat32 && same(*weight),
                            "weight: contiguous float32 (P) on the labels' device expected");
    if (dist2) TORCH_CHECK(dist2->sizes() == idx.sizes() && dist2->scalar_type() == torch::kFloat32 && same(*dist2),
                           "dist2: contiguous float32 (P, K) on the labels' device expected");
    if (share_out) TORCH_CHECK(share_out->dim() == 1 && share_out->size(0) == P && share_out->scalar_type() == torch::kFloat32 && same(*share_out),
                               "share_out: contiguous float32 (P) on the labels' device expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(labels.device());
    const int rc = f3dgs_label_mode_filter((int)P, K, labels.data_ptr<int32_t>(), weight ? weight->data_ptr<float>() : nullptr,
                                           idx.data_ptr<int32_t>(), dist2 ? dist2->data_ptr<float>() : nullptr, (float)max_dist2, fill ? 1 : 0,
                                           labels_out.data_ptr<int32_t>(), share_out ? share_out->data_ptr<float>() : nullptr,
                                           current_stream(labels));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("label_mode_filter: ") + f3dgs_last_error());
}

}  // namespace

PYBIND11_MODULE(_C, m) {
    m.def("distCUDA2", &distCUDA2);
    m.def("knn_neighbors", &knn_neighbors);
    m.def("label_mode_filter", &label_mode_filter);
    m.attr("KNN_MAX_NEIGHBORS") = F3DGS_KNN_MAX_NEIGHBORS;
}
