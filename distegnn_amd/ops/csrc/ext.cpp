// Python bindings for the distegnn_amd gfx950 HIP kernels.
#include <torch/extension.h>

torch::Tensor segment_reduce_csr(torch::Tensor data, torch::Tensor rowptr,
                                 bool mean);
torch::Tensor segment_reduce_csr_perm(torch::Tensor data,
                                      torch::Tensor rowptr,
                                      torch::Tensor perm, bool mean);
torch::Tensor gather_rows_fast(torch::Tensor data, torch::Tensor idx);
torch::Tensor mid_reduce(torch::Tensor x, double scale);
torch::Tensor mid_expand(torch::Tensor g, int64_t c, double scale);
torch::Tensor segment_reduce_chunked(torch::Tensor data, torch::Tensor rowptr,
                                     torch::Tensor chunk_begin,
                                     torch::Tensor chunk_end,
                                     torch::Tensor seg_chunk_ptr, bool mean);
std::vector<torch::Tensor> segment_reduce_chunked_group(
    std::vector<torch::Tensor> tensors, torch::Tensor rowptr,
    torch::Tensor chunk_begin, torch::Tensor chunk_end,
    torch::Tensor seg_chunk_ptr, std::vector<bool> means);
std::vector<torch::Tensor> virtual_aggregate_forward(
    torch::Tensor v_msg, torch::Tensor tv, torch::Tensor tx,
    torch::Tensor rowptr, torch::Tensor chunk_begin, torch::Tensor chunk_end,
    torch::Tensor seg_chunk_ptr);
std::vector<torch::Tensor> virtual_aggregate_backward(
    torch::Tensor dagg_v, torch::Tensor dtrans_v, torch::Tensor dagg_vf,
    torch::Tensor dagg_vc, torch::Tensor batch, torch::Tensor rowptr);
std::tuple<torch::Tensor, torch::Tensor> radius_graph_gpu(torch::Tensor pos,
                                                          double r);
std::tuple<torch::Tensor, torch::Tensor> fused_edge_forward(
    torch::Tensor h, torch::Tensor coord, torch::Tensor eattr,
    torch::Tensor row, torch::Tensor col, torch::Tensor w1, torch::Tensor b1,
    torch::Tensor w2, torch::Tensor b2, torch::Tensor w3, torch::Tensor b3,
    torch::Tensor w3v, bool normalize, double eps,
    std::vector<torch::Tensor> prepped = {});
torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor bt);
torch::Tensor coord_update_forward(torch::Tensor coord, torch::Tensor agg,
                                   torch::Tensor trans_v,
                                   torch::Tensor phiv, torch::Tensor vel);
torch::Tensor coord_update_backward(torch::Tensor g, torch::Tensor vel);
torch::Tensor edge_softmax_fwd(torch::Tensor scores, torch::Tensor dstptr,
                               torch::Tensor perm);
torch::Tensor cfconv_forward(torch::Tensor xw1, torch::Tensor dist,
                             torch::Tensor row, torch::Tensor col,
                             torch::Tensor w1f, torch::Tensor b1,
                             torch::Tensor w2f, torch::Tensor b2,
                             torch::Tensor offsets, double coeff,
                             double cutoff);
torch::Tensor wgrad_splitk_launch(torch::Tensor g, torch::Tensor x);
std::vector<torch::Tensor> wgrad_splitk_group_launch(
    std::vector<torch::Tensor> gs, std::vector<torch::Tensor> xs);
std::tuple<int64_t, int64_t, int64_t> wgrad_plan(int64_t m, int64_t i_dim);
torch::Tensor tall_linear(torch::Tensor x, torch::Tensor bmat,
                          c10::optional<torch::Tensor> bias, int64_t act);
std::vector<torch::Tensor> fused_virtual_forward(
    torch::Tensor h, torch::Tensor coord, torch::Tensor vcoord,
    torch::Tensor vfeat, torch::Tensor gram, torch::Tensor batch,
    torch::Tensor w1, torch::Tensor b1, torch::Tensor w2, torch::Tensor b2,
    torch::Tensor wxv, torch::Tensor bxv, torch::Tensor wxvv,
    torch::Tensor wX, torch::Tensor bX, torch::Tensor wXv, bool train,
    std::vector<torch::Tensor> prepped = {});
std::vector<torch::Tensor> fused_virtual_backward(
    torch::Tensor coord, torch::Tensor vcoord, torch::Tensor batch,
    torch::Tensor dvmsg, torch::Tensor dtv, torch::Tensor dtx,
    torch::Tensor z1, torch::Tensor z2, torch::Tensor zxv, torch::Tensor zX,
    torch::Tensor p2, torch::Tensor w1, torch::Tensor w2, torch::Tensor wxv,
    torch::Tensor wX, torch::Tensor wxvv, torch::Tensor wXv,
    std::vector<torch::Tensor> prepped = {});
std::vector<torch::Tensor> fused_edge_backward(
    torch::Tensor h, torch::Tensor coord, torch::Tensor eattr,
    torch::Tensor row, torch::Tensor col, torch::Tensor dmsg_n,
    torch::Tensor dtrans_n, torch::Tensor w1, torch::Tensor b1,
    torch::Tensor w2, torch::Tensor b2, torch::Tensor w3, torch::Tensor b3,
    torch::Tensor w3v, bool normalize, double eps,
    std::vector<torch::Tensor> prepped = {});
std::vector<torch::Tensor> fused_edge_backward_lin(
    torch::Tensor h, torch::Tensor coord, torch::Tensor eattr,
    torch::Tensor row, torch::Tensor col, torch::Tensor dmsg_n,
    torch::Tensor dtrans_n, torch::Tensor w1, torch::Tensor b1,
    torch::Tensor w2, torch::Tensor b2, torch::Tensor w3, torch::Tensor b3,
    torch::Tensor w3v, bool normalize, double eps,
    std::vector<torch::Tensor> prepped = {});
std::vector<torch::Tensor> segment_reduce_csr_split(
    torch::Tensor data, torch::Tensor rowptr,
    c10::optional<torch::Tensor> perm, c10::optional<torch::Tensor> hi_out,
    c10::optional<torch::Tensor> lo_out);

std::tuple<torch::Tensor, torch::Tensor> fused_edge_forward_f32(
    torch::Tensor h, torch::Tensor coord, torch::Tensor eattr,
    torch::Tensor row, torch::Tensor col, torch::Tensor w1, torch::Tensor b1,
    torch::Tensor w2, torch::Tensor b2, torch::Tensor w3, torch::Tensor b3,
    torch::Tensor w3v, bool normalize, double eps,
    std::vector<torch::Tensor> prepped = {});
torch::Tensor mfma_probe_f32(torch::Tensor a, torch::Tensor bt);
std::vector<torch::Tensor> fused_virtual_forward_f32(
    torch::Tensor h, torch::Tensor coord, torch::Tensor vcoord,
    torch::Tensor vfeat, torch::Tensor gram, torch::Tensor batch,
    torch::Tensor w1, torch::Tensor b1, torch::Tensor w2, torch::Tensor b2,
    torch::Tensor wxv, torch::Tensor bxv, torch::Tensor wxvv,
    torch::Tensor wX, torch::Tensor bX, torch::Tensor wXv,
    std::vector<torch::Tensor> prepped = {});
std::vector<torch::Tensor> fused_node_forward(
    torch::Tensor h, torch::Tensor agg_e, torch::Tensor agg_v,
    c10::optional<torch::Tensor> attr, std::vector<torch::Tensor> prepped,
    bool vel_only);
std::vector<torch::Tensor> fused_node_backward(
    torch::Tensor dh_out, torch::Tensor dphiv, torch::Tensor h,
    torch::Tensor agg_e, torch::Tensor agg_v,
    c10::optional<torch::Tensor> attr, std::vector<torch::Tensor> prepped,
    bool vel_only);
std::vector<torch::Tensor> fused_node_forward_f32(
    torch::Tensor h, c10::optional<torch::Tensor> agg_e,
    c10::optional<torch::Tensor> agg_v, c10::optional<torch::Tensor> attr,
    c10::optional<torch::Tensor> w1, c10::optional<torch::Tensor> b1,
    c10::optional<torch::Tensor> w2, c10::optional<torch::Tensor> b2,
    torch::Tensor wv1, torch::Tensor bv1, torch::Tensor wv2,
    torch::Tensor bv2, bool vel_only,
    std::vector<torch::Tensor> prepped = {});

torch::Tensor radius_graph(torch::Tensor pos, double r) {
  return std::get<0>(radius_graph_gpu(pos, r));
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "distegnn_amd hand-written HIP/CDNA4 kernels (gfx950)";
  m.def("segment_reduce_csr", &segment_reduce_csr,
        "deterministic CSR segmented sum/mean", py::arg("data"),
        py::arg("rowptr"), py::arg("mean"));
  m.def("segment_reduce_csr_perm", &segment_reduce_csr_perm,
        "CSR segmented sum/mean over permuted rows (data[perm[k]])",
        py::arg("data"), py::arg("rowptr"), py::arg("perm"), py::arg("mean"));
  m.def("gather_rows_fast", &gather_rows_fast,
        "vectorized dst[i] = src[idx[i]] row gather", py::arg("data"),
        py::arg("idx"));
  m.def("mid_reduce", &mid_reduce,
        "scale * sum over the middle dim of [N,C,F]", py::arg("x"),
        py::arg("scale"));
  m.def("mid_expand", &mid_expand,
        "broadcast [N,F] over a middle dim: [N,C,F] * scale", py::arg("g"),
        py::arg("c"), py::arg("scale"));
  m.def("segment_reduce_chunked", &segment_reduce_chunked,
        "two-stage deterministic segmented reduce for huge segments",
        py::arg("data"), py::arg("rowptr"), py::arg("chunk_begin"),
        py::arg("chunk_end"), py::arg("seg_chunk_ptr"), py::arg("mean"));
  m.def("segment_reduce_chunked_group", &segment_reduce_chunked_group,
        "segment_reduce_chunked for several operands (contiguous or "
        "row-strided views) in one stage-1 and one combine launch; each "
        "result is bit-equal to segment_reduce_chunked on that operand",
        py::arg("tensors"), py::arg("rowptr"), py::arg("chunk_begin"),
        py::arg("chunk_end"), py::arg("seg_chunk_ptr"), py::arg("means"));
  m.def("virtual_aggregate_forward", &virtual_aggregate_forward,
        "channel means and graph-mean pools of the virtual block outputs: "
        "{agg_v [N,H], trans_v [N,3], agg_vf [B,C,H], agg_vc [B,C,3]}",
        py::arg("v_msg"), py::arg("tv"), py::arg("tx"), py::arg("rowptr"),
        py::arg("chunk_begin"), py::arg("chunk_end"),
        py::arg("seg_chunk_ptr"));
  m.def("virtual_aggregate_backward", &virtual_aggregate_backward,
        "cotangents {dv_msg [N,C,H], dtv [N,C,3], dtx [N,C,3]} of "
        "virtual_aggregate_forward in one kernel",
        py::arg("dagg_v"), py::arg("dtrans_v"), py::arg("dagg_vf"),
        py::arg("dagg_vc"), py::arg("batch"), py::arg("rowptr"));
  m.def("radius_graph_gpu", &radius_graph_gpu,
        "cell-list radius graph -> (edge_index, rowptr)", py::arg("pos"),
        py::arg("r"));
  m.def("radius_graph", &radius_graph, "cell-list radius graph edge_index",
        py::arg("pos"), py::arg("r"));
  m.def("fused_edge_forward", &fused_edge_forward,
        "fused MFMA edge block: gather + phi_e MLP + phi_x head + trans",
        py::arg("h"), py::arg("coord"), py::arg("eattr"), py::arg("row"),
        py::arg("col"), py::arg("w1"), py::arg("b1"), py::arg("w2"),
        py::arg("b2"), py::arg("w3"), py::arg("b3"), py::arg("w3v"),
        py::arg("normalize"), py::arg("eps"),
        py::arg("prepped") = std::vector<torch::Tensor>{});
  m.def("fused_edge_backward", &fused_edge_backward,
        "fused edge-block backward: in-LDS recompute + per-edge grads",
        py::arg("h"), py::arg("coord"), py::arg("eattr"), py::arg("row"),
        py::arg("col"), py::arg("dmsg_n"), py::arg("dtrans_n"),
        py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
        py::arg("w3"), py::arg("b3"), py::arg("w3v"), py::arg("normalize"),
        py::arg("eps"),
        py::arg("prepped") = std::vector<torch::Tensor>{});
  m.def("fused_edge_backward_lin", &fused_edge_backward_lin,
        "edge-block backward for the node-sum path: no ein, dh_row or "
        "dh_col; {t1, msg, dz1, dz2, dz3, dcd, dw3v, gb, gw1_tail [H,3]}",
        py::arg("h"), py::arg("coord"), py::arg("eattr"), py::arg("row"),
        py::arg("col"), py::arg("dmsg_n"), py::arg("dtrans_n"),
        py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
        py::arg("w3"), py::arg("b3"), py::arg("w3v"), py::arg("normalize"),
        py::arg("eps"),
        py::arg("prepped") = std::vector<torch::Tensor>{});
  m.def("segment_reduce_csr_split", &segment_reduce_csr_split,
        "CSR segmented sum of bf16 rows (optionally data[perm[k]]) whose "
        "fp32 result is emitted as two bf16 halves: hi = bf16(S), bit-equal "
        "to segment_reduce_csr, and lo = bf16(S - hi). hi_out / lo_out may "
        "be [n, f] column slices of wider buffers",
        py::arg("data"), py::arg("rowptr"), py::arg("perm") = c10::nullopt,
        py::arg("hi_out") = c10::nullopt, py::arg("lo_out") = c10::nullopt);
  m.def("wgrad_splitk", &wgrad_splitk_launch,
        "split-K MFMA weight gradient: g^T @ x for tall activations",
        py::arg("g"), py::arg("x"));
  m.def("wgrad_splitk_group", &wgrad_splitk_group_launch,
        "up to four split-K weight gradients (g_p^T @ x_p) in one call: one "
        "split-K launch per kernel template, one combine launch; each result "
        "is bit-equal to wgrad_splitk on the same operands",
        py::arg("gs"), py::arg("xs"));
  m.def("wgrad_plan", &wgrad_plan,
        "split plan of wgrad_splitk for [m, 64] x [m, i_dim]: "
        "(chunk_rows, n_slabs, round_rows)",
        py::arg("m"), py::arg("i_dim"));
  m.def("tall_linear", &tall_linear,
        "tall-skinny MFMA linear: act(x @ B^T + bias)",
        py::arg("x"), py::arg("bmat"), py::arg("bias") = c10::nullopt,
        py::arg("act") = 0);
  m.def("fused_virtual_forward", &fused_virtual_forward,
        "fused MFMA virtual-edge block forward");
  m.def("fused_virtual_backward", &fused_virtual_backward,
        "fused MFMA virtual-edge block backward");
  m.def("coord_update_forward", &coord_update_forward,
        "fused coord + agg + trans_v + phi_v*vel");
  m.def("coord_update_backward", &coord_update_backward,
        "dphiv = sum_d g*vel for the fused coordinate update");
  m.def("edge_softmax_fwd", &edge_softmax_fwd,
        "CSR edge softmax over destination segments (SE(3) attention)",
        py::arg("scores"), py::arg("dstptr"), py::arg("perm"));
  m.def("cfconv_forward", &cfconv_forward,
        "fused SchNet CFConv messages: smearing + filter MLP + cutoff + "
        "gathered multiply");
  m.def("mfma_probe", &mfma_probe,
        "16x16x32 bf16 MFMA layout probe: D = A @ B (bt = B^T)",
        py::arg("a"), py::arg("bt"));
  m.def("mfma_probe_f32", &mfma_probe_f32,
        "16x16x4 f32 MFMA layout probe: D = A @ B (a [16,4], bt = B^T [16,4])",
        py::arg("a"), py::arg("bt"));
  m.def("fused_edge_forward_f32", &fused_edge_forward_f32,
        "forward-only fp32 fused edge block (f32 MFMA): {msg [M,H], "
        "trans [M,3]}, both fp32, bitwise reproducible",
        py::arg("h"), py::arg("coord"), py::arg("eattr"), py::arg("row"),
        py::arg("col"), py::arg("w1"), py::arg("b1"), py::arg("w2"),
        py::arg("b2"), py::arg("w3"), py::arg("b3"), py::arg("w3v"),
        py::arg("normalize"), py::arg("eps"),
        py::arg("prepped") = std::vector<torch::Tensor>{});
  m.def("fused_virtual_forward_f32", &fused_virtual_forward_f32,
        "forward-only fp32 fused virtual-edge block (f32 MFMA): {vmsg "
        "[N*C,H], tv [N*C,3], tx [N*C,3]}, all fp32, bitwise reproducible",
        py::arg("h"), py::arg("coord"), py::arg("vcoord"), py::arg("vfeat"),
        py::arg("gram"), py::arg("batch"), py::arg("w1"), py::arg("b1"),
        py::arg("w2"), py::arg("b2"), py::arg("wxv"), py::arg("bxv"),
        py::arg("wxvv"), py::arg("wX"), py::arg("bX"), py::arg("wXv"),
        py::arg("prepped") = std::vector<torch::Tensor>{});
  m.def("fused_node_forward", &fused_node_forward,
        "fused node block forward (bf16 MFMA): phi_h with residual and "
        "phi_v -> {h_out [N,H] bf16, phiv [N,1] fp32}; vel_only computes "
        "phiv alone",
        py::arg("h"), py::arg("agg_e"), py::arg("agg_v"), py::arg("attr"),
        py::arg("prepped"), py::arg("vel_only"));
  m.def("fused_node_backward", &fused_node_backward,
        "fused node block backward: {dh, dagg_e, dagg_v, dz1, t1, dzv "
        "[N,H] bf16, partial rows of the bias/head/attribute gradients}",
        py::arg("dh_out"), py::arg("dphiv"), py::arg("h"), py::arg("agg_e"),
        py::arg("agg_v"), py::arg("attr"), py::arg("prepped"),
        py::arg("vel_only"));
  m.def("fused_node_forward_f32", &fused_node_forward_f32,
        "forward-only fp32 fused node block (f32 MFMA): phi_h with residual "
        "and phi_v -> {h_out [N,H], phiv [N,1]}, both fp32, bitwise "
        "reproducible; vel_only computes phiv alone (h_out is empty) and "
        "reads h and the coord_mlp_vel weights only",
        py::arg("h"), py::arg("agg_e"), py::arg("agg_v"), py::arg("attr"),
        py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
        py::arg("wv1"), py::arg("bv1"), py::arg("wv2"), py::arg("bv2"),
        py::arg("vel_only"),
        py::arg("prepped") = std::vector<torch::Tensor>{});
}
