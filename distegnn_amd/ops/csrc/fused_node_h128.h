// Launchers of the H = 128 fused node block (fused_node_h128.hip). The
// entry points in fused_node.hip validate the arguments, allocate the
// outputs and hand over here when hidden_nf is 128 and N > 0.
#pragma once

#include <torch/extension.h>

#include <vector>

// a = node_attr_nf (0..8); attr is read only when a > 0 and !vel_only.
void fused_node_h128_forward(const torch::Tensor& h,
                             const torch::Tensor& agg_e,
                             const torch::Tensor& agg_v,
                             const c10::optional<torch::Tensor>& attr, int a,
                             const std::vector<torch::Tensor>& prepped,
                             bool vel_only, torch::Tensor& h_out,
                             torch::Tensor& phiv);

// Returns the fp32 partial rows [blocks, 4H + H*A + 1] (one row per block).
torch::Tensor fused_node_h128_backward(
    const torch::Tensor& dh_out, const torch::Tensor& dphiv,
    const torch::Tensor& h, const torch::Tensor& agg_e,
    const torch::Tensor& agg_v, const c10::optional<torch::Tensor>& attr,
    int a, const std::vector<torch::Tensor>& prepped, bool vel_only,
    torch::Tensor& dh, torch::Tensor& dagg_e, torch::Tensor& dagg_v,
    torch::Tensor& dz1, torch::Tensor& t1, torch::Tensor& dzv);
