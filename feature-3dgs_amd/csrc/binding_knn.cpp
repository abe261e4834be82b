// binding_knn.cpp - `simple_knn._C`: the reference's second native module (submodules/simple-knn/ext.cpp:15-17,
// spatial.cu:15-25) on top of the C ABI of libf3dgs_hip.so (include/f3dgs.h: f3dgs_knn_mean_dist2).
//   distCUDA2(points (P,3) float32 on the GPU) -> (P,) float32: mean squared distance to the 3 nearest neighbours.
// Beside it, with no counterpart in the reference (neighbors.py is their Python surface):
//   knn_neighbors(points, K, want_dist2) -> (idx (P,K) int32, dist2 (P,K) float32 or None): f3dgs_knn_neighbors
//   label_mode_filter(labels, weight, idx, dist2, max_dist2, fill, labels_out, share_out): one step of f3dgs_label_mode_filter
//   knn_components(idx, dist2, max_dist2, labels, mutual, dense) -> (root, size, comp, comp_root, n_comp, status): f3dgs_knn_components
//   component_filter(labels, root, size, min_size, largest, num_labels, labels_out): f3dgs_component_filter
//   radius_count(points, radius2, labels, cap) -> count (P,) int32: f3dgs_radius_count
//   knn_outliers(idx, dist2, labels, num_groups, ratio) -> (score (P,) float32, keep (P,) bool, stats (G, 4) float64): f3dgs_knn_outliers
//   group_stats(groups, xyz, G, weight, features, want) -> (count, mass, centroid, cov, aabb, feature_mean), each or None: f3dgs_group_stats
//   group_merge(groups, idx, dist2, max_dist2, mutual, feature_mean, min_cos, out) -> (groups_out, group_root, status): f3dgs_group_merge
//   transform_gaussians(groups, quat, scale, translation, pivot, xyz, rotations, scales, linear, cov3d, sh_rest, rows, inplace)
//       -> (xyz, rotations, scales, cov3d, sh_rest, status), each of the first five or None: f3dgs_transform_gaussians
//   codebook_assign(features, centroids, flags, prev_codes, weight, codes_out, want_dist2, inertia_out, moved_out) -> (codes, dist2 or None):
//       f3dgs_codebook_assign; codebook_update(features, codes, weight, centroids, flags, iteration, count_out): f3dgs_codebook_update, in place;
//       codebook_workspace_bytes(K, C)
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <stdexcept>
#include <string>
#include <vector>

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

// f3dgs_radius_count: count (P) int32; labels: contiguous int32 (P) or None; cap: 0 = no cap
torch::Tensor radius_count(const torch::Tensor& points, double radius2, const c10::optional<torch::Tensor>& labels, int cap) {
    TORCH_CHECK(points.is_cuda(), "points must live on a HIP device: the radius count has no CPU path");
    TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "points must have dimensions (num_points, 3)");
    TORCH_CHECK(points.scalar_type() == torch::kFloat32, "points must be float32");
    TORCH_CHECK(points.size(0) <= (1ll << 30), "too many points");
    TORCH_CHECK(radius2 >= 0.0, "radius2 = ", radius2, ": a squared radius >= 0 expected");
    TORCH_CHECK(cap >= 0, "cap = ", cap, ": 0 (no cap) or a positive count expected");
    const long long P = points.size(0);
    if (labels) check_node_array(*labels, P, points.device(), "labels");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(points.device());
    auto pts = points.contiguous();
    torch::Tensor count = torch::empty({P}, points.options().dtype(torch::kInt32));
    if (P == 0) return count;
    torch::Tensor scratch = torch::empty({(long long)f3dgs_radius_count_scratch_bytes((int)P)}, points.options().dtype(torch::kByte));
    const int rc = f3dgs_radius_count((int)P, pts.data_ptr<float>(), (float)radius2, labels ? labels->data_ptr<int32_t>() : nullptr, cap,
                                      count.data_ptr<int32_t>(), scratch.data_ptr(), current_stream(points));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("radius_count: ") + f3dgs_last_error());
    return count;
}

// f3dgs_knn_outliers: (score (P) float32, keep (P) bool, stats (num_groups, 4) float64).  Nothing is read back.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> knn_outliers(const torch::Tensor& idx, const torch::Tensor& dist2,
                                                                     const c10::optional<torch::Tensor>& labels, int num_groups,
                                                                     double ratio) {
    TORCH_CHECK(idx.is_cuda(), "idx must live on a HIP device: the outlier scores have no CPU path");
    TORCH_CHECK(idx.dim() == 2 && idx.scalar_type() == torch::kInt32 && idx.is_contiguous(), "idx: contiguous int32 (P, K) expected");
    TORCH_CHECK(idx.size(0) <= (1ll << 30), "too many points");
    const long long P = idx.size(0);
    const int K = (int)idx.size(1);
    TORCH_CHECK(dist2.sizes() == idx.sizes() && dist2.scalar_type() == torch::kFloat32 && dist2.device() == idx.device() &&
                    dist2.is_contiguous(), "dist2: contiguous float32 (P, K) on the lists' device expected");
    if (labels) check_node_array(*labels, P, idx.device(), "labels");
    TORCH_CHECK(num_groups >= 1 && (labels || num_groups == 1), "num_groups = ", num_groups, ": >= 1, and 1 without labels");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(idx.device());
    torch::Tensor score = torch::empty({P}, dist2.options());
    torch::Tensor keep = torch::empty({P}, idx.options().dtype(torch::kBool));
    torch::Tensor stats = torch::empty({(long long)num_groups, 4}, idx.options().dtype(torch::kFloat64));
    torch::Tensor scratch = torch::empty({(long long)f3dgs_knn_outliers_scratch_bytes(num_groups)}, idx.options().dtype(torch::kByte));
    // (an empty tensor has no address: with P == 0 nothing is read or written through these)
    const int rc = f3dgs_knn_outliers((int)P, K, P > 0 ? idx.data_ptr<int32_t>() : nullptr, P > 0 ? dist2.data_ptr<float>() : nullptr,
                                      (labels && P > 0) ? labels->data_ptr<int32_t>() : nullptr, num_groups, (float)ratio,
                                      P > 0 ? score.data_ptr<float>() : nullptr, stats.data_ptr<double>(),
                                      P > 0 ? static_cast<uint8_t*>(keep.data_ptr()) : nullptr, scratch.data_ptr(), current_stream(idx));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("knn_outliers: ") + f3dgs_last_error());
    return {score, keep, stats};
}

// f3dgs_group_stats: `want` names the outputs (GROUP_COUNT ... GROUP_FEATURE_MEAN); the others come back as None.  count (G) int32,
// mass (G), centroid (G, 3), cov (G, 6), aabb (G, 6), feature_mean (G, C) float32.  features: (P, C) float32 with unit stride along
// C and any row stride >= C (a view is read in place).  Nothing is read back.
enum { GROUP_COUNT = 1, GROUP_MASS = 2, GROUP_CENTROID = 4, GROUP_COV = 8, GROUP_AABB = 16, GROUP_FEATURE_MEAN = 32 };

std::vector<c10::optional<torch::Tensor>> group_stats(const torch::Tensor& groups, const torch::Tensor& xyz, int G,
                                                      const c10::optional<torch::Tensor>& weight,
                                                      const c10::optional<torch::Tensor>& features, int want) {
    TORCH_CHECK(groups.is_cuda(), "groups must live on a HIP device: the group statistics have no CPU path");
    TORCH_CHECK(groups.dim() == 1 && groups.scalar_type() == torch::kInt32 && groups.is_contiguous(), "groups: contiguous int32 (P) expected");
    const long long P = groups.size(0);
    TORCH_CHECK(P < (1ll << 31), "too many points");
    const auto dev = groups.device();
    TORCH_CHECK(xyz.dim() == 2 && xyz.size(0) == P && xyz.size(1) == 3 && xyz.scalar_type() == torch::kFloat32 && xyz.device() == dev &&
                    xyz.is_contiguous(), "xyz: contiguous float32 (P, 3) on the groups' device expected");
    TORCH_CHECK(G >= 1 && G <= F3DGS_GROUP_MAX_GROUPS, "G = ", G, ": 1 .. ", F3DGS_GROUP_MAX_GROUPS, " groups are taken");
    if (weight) TORCH_CHECK(weight->dim() == 1 && weight->size(0) == P && weight->scalar_type() == torch::kFloat32 && weight->device() == dev &&
                                weight->is_contiguous(), "weight: contiguous float32 (P) on the groups' device expected");
    int C = 0;
    long long stride = 0;
    if (features) {
        TORCH_CHECK(features->dim() == 2 && features->size(0) == P && features->scalar_type() == torch::kFloat32 && features->device() == dev,
                    "features: float32 (P, C) on the groups' device expected");
        TORCH_CHECK(features->size(1) >= 1 && features->size(1) <= F3DGS_GROUP_MAX_CHANNELS, "C = ", features->size(1), ": 1 .. ",
                    F3DGS_GROUP_MAX_CHANNELS, " channels are taken");
        C = (int)features->size(1);
        stride = P > 1 ? features->stride(0) : C;
        TORCH_CHECK(P == 0 || ((C == 1 || features->stride(1) == 1) && stride >= C),
                    "features: unit stride along C and a row stride >= C expected");
    }
    TORCH_CHECK(want > 0 && want < 64, "want = ", want, ": a sum of GROUP_COUNT ... GROUP_FEATURE_MEAN expected");
    TORCH_CHECK(!(want & GROUP_FEATURE_MEAN) || features, "feature_mean needs features");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto floats = xyz.options();
    std::vector<c10::optional<torch::Tensor>> out(6);
    if (want & GROUP_COUNT) out[0] = torch::empty({G}, groups.options());
    if (want & GROUP_MASS) out[1] = torch::empty({G}, floats);
    if (want & GROUP_CENTROID) out[2] = torch::empty({G, 3}, floats);
    if (want & GROUP_COV) out[3] = torch::empty({G, 6}, floats);
    if (want & GROUP_AABB) out[4] = torch::empty({G, 6}, floats);
    if (want & GROUP_FEATURE_MEAN) out[5] = torch::empty({G, C}, floats);
    const size_t bytes = f3dgs_group_stats_scratch_bytes(G, C);
    torch::Tensor scratch = torch::empty({(long long)bytes}, floats.dtype(torch::kByte));
    auto fp = [&](int k) { return out[k] ? out[k]->data_ptr<float>() : nullptr; };
    // (an empty tensor has no address, and C > 0 needs one: with P == 0 nothing is read through it)
    const float* feat = !features ? nullptr : (P > 0 ? features->data_ptr<float>() : static_cast<const float*>(scratch.data_ptr()));
    const int rc = f3dgs_group_stats((int)P, G, C, groups.data_ptr<int32_t>(), xyz.data_ptr<float>(), weight ? weight->data_ptr<float>() : nullptr,
                                     feat, stride, out[0] ? out[0]->data_ptr<int32_t>() : nullptr,
                                     fp(1), fp(2), fp(3), fp(4), fp(5), scratch.data_ptr(), bytes, current_stream(groups));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("group_stats: ") + f3dgs_last_error());
    return out;
}

// f3dgs_group_merge: (groups_out (P), group_root (G), status), int32; `out`: the caller's groups_out (it may be `groups`)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> group_merge(const torch::Tensor& groups, const torch::Tensor& idx,
                                                                    const c10::optional<torch::Tensor>& dist2, double max_dist2, bool mutual,
                                                                    const torch::Tensor& feature_mean, double min_cos,
                                                                    const c10::optional<torch::Tensor>& out) {
    TORCH_CHECK(groups.is_cuda(), "groups must live on a HIP device: the merge has no CPU path");
    TORCH_CHECK(groups.dim() == 1, "groups: contiguous int32 (P) expected");
    const long long P = groups.size(0);
    TORCH_CHECK(P <= (1ll << 30), "too many points");
    const auto dev = groups.device();
    check_node_array(groups, P, dev, "groups");
    TORCH_CHECK(idx.dim() == 2 && idx.size(0) == P && idx.scalar_type() == torch::kInt32 && idx.device() == dev && idx.is_contiguous(),
                "idx: contiguous int32 (P, K) on the groups' device expected");
    const int K = (int)idx.size(1);
    if (dist2) TORCH_CHECK(dist2->sizes() == idx.sizes() && dist2->scalar_type() == torch::kFloat32 && dist2->device() == dev &&
                               dist2->is_contiguous(), "dist2: contiguous float32 (P, K) on the groups' device expected");
    TORCH_CHECK(feature_mean.dim() == 2 && feature_mean.scalar_type() == torch::kFloat32 && feature_mean.device() == dev &&
                    feature_mean.is_contiguous(), "feature_mean: contiguous float32 (G, C) on the groups' device expected");
    TORCH_CHECK(feature_mean.size(0) >= 1 && feature_mean.size(0) <= F3DGS_GROUP_MERGE_MAX_GROUPS, "G = ", feature_mean.size(0), ": 1 .. ",
                F3DGS_GROUP_MERGE_MAX_GROUPS, " groups are taken");
    TORCH_CHECK(feature_mean.size(1) >= 1 && feature_mean.size(1) <= F3DGS_GROUP_MAX_CHANNELS, "C = ", feature_mean.size(1), ": 1 .. ",
                F3DGS_GROUP_MAX_CHANNELS, " channels are taken");
    const int G = (int)feature_mean.size(0), C = (int)feature_mean.size(1);
    if (out) check_node_array(*out, P, dev, "out");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto ints = groups.options();
    torch::Tensor groups_out = out ? *out : torch::empty({P}, ints);
    torch::Tensor group_root = torch::empty({G}, ints), status = torch::empty({}, ints);
    const size_t bytes = f3dgs_group_merge_scratch_bytes(G);
    torch::Tensor scratch = torch::empty({(long long)bytes}, ints.dtype(torch::kByte));
    const int rc = f3dgs_group_merge((int)P, K, G, C, groups.data_ptr<int32_t>(), idx.data_ptr<int32_t>(), dist2 ? dist2->data_ptr<float>() : nullptr,
                                     (float)max_dist2, mutual ? 1 : 0, feature_mean.data_ptr<float>(), (float)min_cos,
                                     group_root.data_ptr<int32_t>(), groups_out.data_ptr<int32_t>(), status.data_ptr<int32_t>(),
                                     scratch.data_ptr(), bytes, current_stream(groups));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("group_merge: ") + f3dgs_last_error());
    return {groups_out, group_root, status};
}

// f3dgs_transform_gaussians.  The table: quat (G, 4), scale (G), translation (G, 3), pivot (G, 3) or None, contiguous float32.
// Per-Gaussian tensors, each or None: xyz (P, 3), rotations (P, 4), scales (P, 3), cov3d (P, 6) contiguous float32; sh_rest
// (P, n_rest, 3) float32, n_rest in {3, 8, 15}, contiguous in its last two dimensions with any row stride >= 3 n_rest (a view is
// read in place).  rows: (M) int32 or None (the gather form).  inplace: the outputs ARE the inputs (not with rows).  Returns the
// transformed tensors in the order of the arguments (None where none was given) and status (G) int32.  Nothing is read back.
std::vector<c10::optional<torch::Tensor>> transform_gaussians(const torch::Tensor& groups, const torch::Tensor& quat, const torch::Tensor& scale,
                                                              const torch::Tensor& translation, const c10::optional<torch::Tensor>& pivot,
                                                              const c10::optional<torch::Tensor>& xyz,
                                                              const c10::optional<torch::Tensor>& rotations,
                                                              const c10::optional<torch::Tensor>& scales, bool linear,
                                                              const c10::optional<torch::Tensor>& cov3d,
                                                              const c10::optional<torch::Tensor>& sh_rest,
                                                              const c10::optional<torch::Tensor>& rows, bool inplace) {
    TORCH_CHECK(groups.is_cuda(), "groups must live on a HIP device: the object transforms have no CPU path");
    TORCH_CHECK(groups.dim() == 1 && groups.scalar_type() == torch::kInt32 && groups.is_contiguous(), "groups: contiguous int32 (P) expected");
    const long long P = groups.size(0);
    TORCH_CHECK(P <= (1ll << 30), "too many points");
    const auto dev = groups.device();
    auto is_table = [&](const torch::Tensor& t, long long G, long long w) {
        return t.scalar_type() == torch::kFloat32 && t.device() == dev && t.is_contiguous() &&
               (w == 0 ? (t.dim() == 1 && t.size(0) == G) : (t.dim() == 2 && t.size(0) == G && t.size(1) == w));
    };
    TORCH_CHECK(scale.dim() == 1, "scale: contiguous float32 (G) on the groups' device expected");
    const long long G = scale.size(0);
    TORCH_CHECK(G >= 1 && G <= F3DGS_GROUP_MAX_GROUPS, "G = ", G, ": 1 .. ", F3DGS_GROUP_MAX_GROUPS, " groups are taken");
    TORCH_CHECK(is_table(scale, G, 0), "scale: contiguous float32 (G) on the groups' device expected");
    TORCH_CHECK(is_table(quat, G, 4), "quat: contiguous float32 (G, 4) on the groups' device expected");
    TORCH_CHECK(is_table(translation, G, 3), "translation: contiguous float32 (G, 3) on the groups' device expected");
    if (pivot) TORCH_CHECK(is_table(*pivot, G, 3), "pivot: contiguous float32 (G, 3) on the groups' device expected");
    const c10::optional<torch::Tensor>* in[4] = {&xyz, &rotations, &scales, &cov3d};
    const char* names[4] = {"xyz", "rotations", "scales", "cov3d"};
    const long long width[4] = {3, 4, 3, 6};
    for (int a = 0; a < 4; a++)
        if (*in[a]) TORCH_CHECK(is_table(**in[a], P, width[a]), names[a], ": contiguous float32 (P, ", width[a], ") on the groups' device expected");
    int n_rest = 0;
    long long stride = 0;
    if (sh_rest) {
        TORCH_CHECK(sh_rest->dim() == 3 && sh_rest->size(0) == P && sh_rest->size(2) == 3 && sh_rest->scalar_type() == torch::kFloat32 &&
                        sh_rest->device() == dev, "sh_rest: float32 (P, n_rest, 3) on the groups' device expected");
        TORCH_CHECK(sh_rest->size(1) == 3 || sh_rest->size(1) == 8 || sh_rest->size(1) == 15, "sh_rest: n_rest = ", sh_rest->size(1),
                    ", 3, 8 and 15 are taken");
        n_rest = (int)sh_rest->size(1);
        stride = P > 1 ? sh_rest->stride(0) : 3 * n_rest;
        TORCH_CHECK(P == 0 || (sh_rest->stride(2) == 1 && sh_rest->stride(1) == 3 && stride >= 3 * n_rest),
                    "sh_rest: rows of n_rest x 3 contiguous floats and a row stride >= 3 n_rest expected");
    }
    TORCH_CHECK(xyz || rotations || scales || cov3d || sh_rest, "no per-Gaussian tensor given");
    TORCH_CHECK(!(rows && inplace), "inplace and rows exclude each other");
    long long M = P;
    if (rows) {
        TORCH_CHECK(rows->dim() == 1 && rows->scalar_type() == torch::kInt32 && rows->device() == dev && rows->is_contiguous(),
                    "rows: contiguous int32 (M) on the groups' device expected");
        M = rows->size(0);
        TORCH_CHECK(M < (1ll << 31), "too many rows");
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto floats = quat.options();
    std::vector<c10::optional<torch::Tensor>> out(6);
    for (int a = 0; a < 4; a++)
        if (*in[a]) out[a] = inplace ? **in[a] : torch::empty({M, width[a]}, floats);
    if (sh_rest) out[4] = inplace ? *sh_rest : torch::empty({M, (long long)n_rest, 3}, floats);
    torch::Tensor status = torch::empty({G}, groups.options());
    out[5] = status;
    const size_t bytes = f3dgs_transform_gaussians_scratch_bytes((int)G);
    torch::Tensor scratch = torch::empty({(long long)bytes}, floats.dtype(torch::kByte));
    // (an empty tensor has no address: with P == 0 or M == 0 nothing is read or written through these)
    float* const nowhere = static_cast<float*>(scratch.data_ptr());
    auto ip = [&](const c10::optional<torch::Tensor>& t) -> const float* { return !t ? nullptr : (P > 0 ? t->data_ptr<float>() : nowhere); };
    auto op = [&](int a) -> float* { return !out[a] ? nullptr : (M > 0 && P > 0 ? out[a]->data_ptr<float>() : nowhere + 64); };
    const int rc = f3dgs_transform_gaussians(
        (int)P, (int)G, quat.data_ptr<float>(), scale.data_ptr<float>(), translation.data_ptr<float>(), pivot ? pivot->data_ptr<float>() : nullptr,
        P > 0 ? groups.data_ptr<int32_t>() : nullptr, rows ? (M > 0 ? rows->data_ptr<int32_t>() : reinterpret_cast<const int32_t*>(nowhere)) : nullptr,
        (int)M, ip(xyz), ip(rotations), ip(scales), linear ? F3DGS_TRANSFORM_SCALES_LINEAR : F3DGS_TRANSFORM_SCALES_LOG, ip(cov3d), ip(sh_rest),
        n_rest, stride, op(0), op(1), op(2), op(3), op(4), inplace ? stride : 3 * n_rest, status.data_ptr<int32_t>(), scratch.data_ptr(), bytes,
        current_stream(groups));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("transform_gaussians: ") + f3dgs_last_error());
    return out;
}

// the (P, C) features of the codebook entries: float32, unit stride along C, any row stride >= C (a view is read in place)
long long codebook_features(const torch::Tensor& features, long long* P, int* C) {
    TORCH_CHECK(features.is_cuda(), "features must live on a HIP device: the codebooks have no CPU path");
    TORCH_CHECK(features.dim() == 2 && features.scalar_type() == torch::kFloat32, "features: float32 (P, C) expected");
    TORCH_CHECK(features.size(1) >= 1 && features.size(1) <= F3DGS_CODEBOOK_MAX_CHANNELS, "C = ", features.size(1), ": 1 .. ",
                F3DGS_CODEBOOK_MAX_CHANNELS, " channels are taken");
    *P = features.size(0);
    *C = (int)features.size(1);
    TORCH_CHECK(*P < (1ll << 31) - 129, "too many rows");
    const long long stride = *P > 1 ? features.stride(0) : *C;
    TORCH_CHECK(*P == 0 || ((*C == 1 || features.stride(1) == 1) && stride >= *C), "features: unit stride along C and a row stride >= C expected");
    return stride;
}

void codebook_centroids(const torch::Tensor& centroids, const torch::Tensor& features, int C) {
    TORCH_CHECK(centroids.dim() == 2 && centroids.size(1) == C && centroids.scalar_type() == torch::kFloat32 &&
                    centroids.device() == features.device() && centroids.is_contiguous(),
                "centroids: contiguous float32 (K, C) on the features' device expected");
    TORCH_CHECK(centroids.size(0) >= 1 && centroids.size(0) <= F3DGS_CODEBOOK_MAX_CENTROIDS, "K = ", centroids.size(0), ": 1 .. ",
                F3DGS_CODEBOOK_MAX_CENTROIDS, " centroids are taken");
}

void codebook_rows(const c10::optional<torch::Tensor>& t, const torch::Tensor& features, long long n, c10::ScalarType type, const char* what) {
    if (!t) return;
    TORCH_CHECK(t->dim() == 1 && t->size(0) == n && t->scalar_type() == type && t->device() == features.device() && t->is_contiguous(), what);
}

// f3dgs_codebook_assign.  codes_out: the caller's (P) int32 (it may be prev_codes) or None; inertia_out: one float64, moved_out: one
// int32 on the device, each or None - a slot of a per-iteration tensor.  Nothing is read back.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> codebook_assign(
    const torch::Tensor& features, const torch::Tensor& centroids, int flags, const c10::optional<torch::Tensor>& prev_codes,
    const c10::optional<torch::Tensor>& weight, const c10::optional<torch::Tensor>& codes_out, bool want_dist2,
    const c10::optional<torch::Tensor>& inertia_out, const c10::optional<torch::Tensor>& moved_out) {
    long long P;
    int C;
    const long long stride = codebook_features(features, &P, &C);
    codebook_centroids(centroids, features, C);
    const int K = (int)centroids.size(0);
    codebook_rows(prev_codes, features, P, torch::kInt32, "prev_codes: contiguous int32 (P) on the features' device expected");
    codebook_rows(codes_out, features, P, torch::kInt32, "codes_out: contiguous int32 (P) on the features' device expected");
    codebook_rows(weight, features, P, torch::kFloat32, "weight: contiguous float32 (P) on the features' device expected");
    codebook_rows(inertia_out, features, 1, torch::kFloat64, "inertia_out: one float64 on the features' device expected");
    codebook_rows(moved_out, features, 1, torch::kInt32, "moved_out: one int32 on the features' device expected");
    TORCH_CHECK(!moved_out || prev_codes, "moved_out needs prev_codes");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(features.device());
    torch::Tensor codes = codes_out ? *codes_out : torch::empty({P}, features.options().dtype(torch::kInt32));
    c10::optional<torch::Tensor> dist2;
    if (want_dist2) dist2 = torch::empty({P}, features.options());
    const size_t bytes = f3dgs_codebook_workspace_bytes(K, C);
    torch::Tensor workspace = torch::empty({(long long)bytes}, features.options().dtype(torch::kByte));
    // (an empty tensor has no address: with P == 0 nothing is read through these)
    const float* feat = P > 0 ? features.data_ptr<float>() : static_cast<const float*>(workspace.data_ptr());
    const int rc = f3dgs_codebook_assign((int)P, K, C, feat, stride, centroids.data_ptr<float>(), flags,
                                         (prev_codes && P > 0) ? prev_codes->data_ptr<int32_t>() : nullptr,
                                         (weight && P > 0) ? weight->data_ptr<float>() : nullptr,
                                         P > 0 ? codes.data_ptr<int32_t>() : nullptr, (dist2 && P > 0) ? dist2->data_ptr<float>() : nullptr,
                                         inertia_out ? inertia_out->data_ptr<double>() : nullptr,
                                         (moved_out && (P > 0 || prev_codes)) ? moved_out->data_ptr<int32_t>() : nullptr, workspace.data_ptr(), bytes,
                                         current_stream(features));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("codebook_assign: ") + f3dgs_last_error());
    return {codes, dist2};
}

// f3dgs_codebook_update: `centroids` (K, C) is moved in place; count_out: the caller's (K) int32 or None
void codebook_update(const torch::Tensor& features, const torch::Tensor& codes, const c10::optional<torch::Tensor>& weight,
                     torch::Tensor centroids, int flags, int iteration, const c10::optional<torch::Tensor>& count_out) {
    long long P;
    int C;
    const long long stride = codebook_features(features, &P, &C);
    codebook_centroids(centroids, features, C);
    const int K = (int)centroids.size(0);
    codebook_rows(codes, features, P, torch::kInt32, "codes: contiguous int32 (P) on the features' device expected");
    codebook_rows(weight, features, P, torch::kFloat32, "weight: contiguous float32 (P) on the features' device expected");
    codebook_rows(count_out, features, K, torch::kInt32, "count_out: contiguous int32 (K) on the features' device expected");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(features.device());
    const size_t bytes = f3dgs_codebook_update_scratch_bytes(K, C);
    torch::Tensor scratch = torch::empty({(long long)bytes}, features.options().dtype(torch::kByte));
    const float* feat = P > 0 ? features.data_ptr<float>() : static_cast<const float*>(scratch.data_ptr());
    const int rc = f3dgs_codebook_update((int)P, K, C, feat, stride, P > 0 ? codes.data_ptr<int32_t>() : nullptr,
                                         (weight && P > 0) ? weight->data_ptr<float>() : nullptr, flags, iteration, centroids.data_ptr<float>(),
                                         count_out ? count_out->data_ptr<int32_t>() : nullptr, scratch.data_ptr(), bytes, current_stream(features));
    if (rc != F3DGS_OK) throw std::runtime_error(std::string("codebook_update: ") + f3dgs_last_error());
}

}  // namespace

PYBIND11_MODULE(_C, m) {
    m.def("distCUDA2", &distCUDA2);
    m.def("knn_neighbors", &knn_neighbors);
    m.def("label_mode_filter", &label_mode_filter);
    m.def("knn_components", &knn_components);
    m.def("component_filter", &component_filter);
    m.def("radius_count", &radius_count);
    m.def("knn_outliers", &knn_outliers);
    m.def("group_stats", &group_stats);
    m.def("group_merge", &group_merge);
    m.def("transform_gaussians", &transform_gaussians);
    m.def("codebook_assign", &codebook_assign);
    m.def("codebook_update", &codebook_update);
    m.def("codebook_workspace_bytes", [](int K, int C) { return (long long)f3dgs_codebook_workspace_bytes(K, C); });
    m.attr("CODEBOOK_COSINE") = F3DGS_CODEBOOK_COSINE;
    m.attr("CODEBOOK_RESEED_EMPTY") = F3DGS_CODEBOOK_RESEED_EMPTY;
    m.attr("CODEBOOK_MAX_CENTROIDS") = F3DGS_CODEBOOK_MAX_CENTROIDS;
    m.attr("CODEBOOK_MAX_CHANNELS") = F3DGS_CODEBOOK_MAX_CHANNELS;
    m.attr("GROUP_COUNT") = (int)GROUP_COUNT;
    m.attr("GROUP_MASS") = (int)GROUP_MASS;
    m.attr("GROUP_CENTROID") = (int)GROUP_CENTROID;
    m.attr("GROUP_COV") = (int)GROUP_COV;
    m.attr("GROUP_AABB") = (int)GROUP_AABB;
    m.attr("GROUP_FEATURE_MEAN") = (int)GROUP_FEATURE_MEAN;
    m.attr("GROUP_MAX_GROUPS") = F3DGS_GROUP_MAX_GROUPS;
    m.attr("GROUP_MAX_CHANNELS") = F3DGS_GROUP_MAX_CHANNELS;
    m.attr("GROUP_MERGE_MAX_GROUPS") = F3DGS_GROUP_MERGE_MAX_GROUPS;
    m.attr("KNN_MAX_NEIGHBORS") = F3DGS_KNN_MAX_NEIGHBORS;
}
