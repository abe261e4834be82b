// binding_knn.cpp - `simple_knn._C`: the reference's second native module (submodules/simple-knn/ext.cpp:15-17,
// spatial.cu:15-25) on top of the C ABI of libf3dgs_hip.so (include/f3dgs.h: f3dgs_knn_mean_dist2).
//   distCUDA2(points (P,3) float32 on the GPU) -> (P,) float32: mean squared distance to the 3 nearest neighbours.
// Beside it, with no counterpart in the reference (neighbors.py is their Python surface):
//   knn_neighbors(points, K, want_dist2) -> (idx (P,K) int32, dist2 (P,K) float32 or None): f3dgs_knn_neighbors
//   label_mode_filter(labels, weight, idx, dist2, max_dist2, fill, labels_out, share_out): one step of f3dgs_label_mode_filter
//   knn_components(idx, dist2, max_dist2, labels, mutual, dense) -> (root, size, comp, comp_root, n_comp, status): f3dgs_knn_components
//   component_filter(labels, root, size, min_size, largest, num_labels, labels_out): f3dgs_component_filter
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

void check_node_array(const torch::Tensor& t, long long P, const torch::Device& dev, const char* name) {
    TORCH_CHECK(t.dim() == 1 && t.size(0) == P && t.scalar_type() == torch::kInt32 && t.device() == dev && t.is_contiguous(), name,
                ": contiguous int32 (P) on the lists' device expected");
}

// f3dgs_knn_components: (root, size, comp, comp_root, n_comp, status), all int32; comp, comp_root (P) and n_comp (a 0-dim tensor)
// only with `dense`; status a 0-dim tensor.  Nothing is read back.
std::tuple<torch::Tensor, torch::Tensor, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, torch::Tensor>
knn_components(const torch::Tensor& idx, const c10::optional<torch::Tensor>& dist2, double max_dist2,
               const c10::optional<torch::Tensor>& labels, bool mutual, bool dense) {
    TORCH_CHECK(idx.is_cuda(), "idx must live on a HIP device: the components have no CPU path");
    TORCH_CHECK(idx.dim() == 2 && idx.scalar_type() == torch::kInt32 && idx.is_contiguous(), "idx: contiguous int32 (P, K) expected");
    TORCH_CHECK(idx.size(0) <= (1ll << 30), "too many points");
    const long long P = idx.size(0);
    const int K = (int)idx.size(1);
    if (dist2) TORCH_CHECK(dist2->sizes() == idx.sizes() && dist2->scalar_type() == torch::kFloat32 && dist2->device() == idx.device() &&
                               dist2->is_contiguous(), "dist2: contiguous float32 (P, K) on the lists' device expected");
    if (labels) check_node_array(*labels, P, idx.device(), "labels");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(idx.device());
    const auto ints = idx.options();
    torch::Tensor root = torch::empty({P}, ints), size = torch::empty({P}, ints), status = torch::empty({}, ints);
    c10::optional<torch::Tensor> comp, comp_root, n_comp;
    torch::Tensor scratch;
    if (dense) {
        comp = torch::empty({P}, ints);
        comp_root = torch::empty({P}, ints);
        n_comp = torch::empty({}, ints);
        scratch = torch::empty({(long long)f3dgs_knn_components_scratch_bytes((int)P, 0)}, ints.dtype(torch::kByte));
    }
    const int rc = f3dgs_knn_components((int)P, K, idx.data_ptr<int32_t>(), dist2 ? dist2->data_ptr<float>() : nullptr, (float)max_dist2,
                                        labels ? labels->data_ptr<int32_t>() : nullptr, mutual ? 1 : 0, root.data_ptr<int32_t>(),
                                        size.data_ptr<int32_t>(), dense ? comp->data_ptr<int32_t>() : nullptr,
                                        dense ? comp_root->data_ptr<int32_t>() : nullptr, dense ? n_comp->data_ptr<int32_t>() : nullptr,
                                        status.data_ptr<int32_t>(), dense ? scratch.data_ptr() : nullptr, current_stream(idx));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("knn_components: ") + f3dgs_last_error());
    return {root, size, comp, comp_root, n_comp, status};
}

// f3dgs_component_filter into the caller's labels_out (which may be labels)
void component_filter(const c10::optional<torch::Tensor>& labels, const torch::Tensor& root, const torch::Tensor& size, int min_size,
                      bool largest, int num_labels, torch::Tensor& labels_out) {
    TORCH_CHECK(root.is_cuda(), "root must live on a HIP device: the component filter has no CPU path");
    TORCH_CHECK(root.dim() == 1, "root: contiguous int32 (P) expected");
    const long long P = root.size(0);
    TORCH_CHECK(P <= (1ll << 30), "too many points");
    check_node_array(root, P, root.device(), "root");
    check_node_array(size, P, root.device(), "size");
    check_node_array(labels_out, P, root.device(), "labels_out");
    if (labels) check_node_array(*labels, P, root.device(), "labels");
    TORCH_CHECK(!largest || num_labels >= 0, "num_labels = ", num_labels, " with largest");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(root.device());
    torch::Tensor scratch;
    if (largest) scratch = torch::empty({(long long)f3dgs_knn_components_scratch_bytes(0, num_labels)}, root.options().dtype(torch::kByte));
    const int rc = f3dgs_component_filter((int)P, labels ? labels->data_ptr<int32_t>() : nullptr, root.data_ptr<int32_t>(),
                                          size.data_ptr<int32_t>(), min_size, largest ? 1 : 0, num_labels, labels_out.data_ptr<int32_t>(),
                                          largest ? scratch.data_ptr() : nullptr, current_stream(root));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("component_filter: ") + f3dgs_last_error());
}

}  // namespace

PYBIND11_MODULE(_C, m) {
    m.def("distCUDA2", &distCUDA2);
    m.def("knn_neighbors", &knn_neighbors);
    m.def("label_mode_filter", &label_mode_filter);
    m.def("knn_components", &knn_components);
    m.def("component_filter", &component_filter);
    m.attr("KNN_MAX_NEIGHBORS") = F3DGS_KNN_MAX_NEIGHBORS;
}
