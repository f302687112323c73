// Python bindings for the megatron_amd CDNA4 HIP kernels.
#include <torch/extension.h>

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w, double eps);
std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w, torch::Tensor rstd,
                                       c10::optional<torch::Tensor> dres);
std::vector<torch::Tensor> add_rmsnorm_fwd(torch::Tensor x, torch::Tensor residual, torch::Tensor w, double eps);
torch::Tensor swiglu_fwd(torch::Tensor x);
torch::Tensor swiglu_bwd(torch::Tensor dy, torch::Tensor x);
torch::Tensor rope_fwd(torch::Tensor x, torch::Tensor cost, torch::Tensor sint);
torch::Tensor rope_bwd(torch::Tensor dy, torch::Tensor cost, torch::Tensor sint);
std::vector<torch::Tensor> qkv_split_rope_fwd(torch::Tensor qkv, torch::Tensor cost, torch::Tensor sint, long rep);
torch::Tensor qkv_split_rope_bwd(torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
                                 torch::Tensor cost, torch::Tensor sint);
void multi_tensor_adamw(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads,
                        std::vector<torch::Tensor> exp_avgs, std::vector<torch::Tensor> exp_avg_sqs,
                        std::vector<torch::Tensor> model_params,
                        double lr, double beta1, double beta2, double eps, double wd, long step);
torch::Tensor multi_tensor_l2norm(std::vector<torch::Tensor> tensors);
void wgrad_gemm_accum(torch::Tensor main_grad, torch::Tensor grad_output, torch::Tensor input);
std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                    bool causal, double scale, long window);
std::vector<torch::Tensor> attn_bwd(torch::Tensor dout, torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor out, torch::Tensor lse,
                                    bool causal, double scale, long window);
std::vector<torch::Tensor> attn_varlen_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                           torch::Tensor cu_seqlens, bool causal, double scale);
std::vector<torch::Tensor> attn_varlen_bwd(torch::Tensor dout, torch::Tensor q, torch::Tensor k,
                                           torch::Tensor v, torch::Tensor out, torch::Tensor lse,
                                           torch::Tensor cu_seqlens, bool causal, double scale);
torch::Tensor attn_paged_decode(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                                torch::Tensor block_tables, torch::Tensor lens, double scale,
                                c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale);
torch::Tensor attn_paged_prefill(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                                 torch::Tensor block_table, long prior_len, double scale, long window,
                                 c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale);
std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor target, long vocab_start);
void ce_bwd(torch::Tensor logits, torch::Tensor target, torch::Tensor row_max,
            torch::Tensor row_inv_sumexp, torch::Tensor grad_out, long vocab_start);
std::string grouped_gemm_probe();
torch::Tensor grouped_gemm(torch::Tensor a, torch::Tensor b, std::vector<int64_t> sizes, bool trans_b);
void grouped_gemm_wgrad(torch::Tensor dy, torch::Tensor x, std::vector<int64_t> sizes, torch::Tensor dw);
torch::Tensor grouped_gemm_hip(torch::Tensor a, torch::Tensor b, torch::Tensor sizes, bool trans_b);
void grouped_gemm_hip_wgrad(torch::Tensor dy, torch::Tensor x, torch::Tensor sizes, torch::Tensor dw,
                            bool accumulate);
std::vector<torch::Tensor> mx_quantize(torch::Tensor t, bool dual);
torch::Tensor mx_gemm_nt(torch::Tensor aq, torch::Tensor a_s, torch::Tensor bq, torch::Tensor b_s);
std::vector<torch::Tensor> causal_conv1d_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor bias);
std::vector<torch::Tensor> causal_conv1d_bwd(torch::Tensor dy, torch::Tensor x,
                                             torch::Tensor pre, torch::Tensor w);
std::vector<torch::Tensor> ssd_scan_fwd(torch::Tensor x, torch::Tensor dt, torch::Tensor A, torch::Tensor B,
                                        torch::Tensor C, c10::optional<torch::Tensor> D,
                                        c10::optional<torch::Tensor> initial_state);
torch::Tensor ssd_step_fwd(torch::Tensor x, torch::Tensor dt, torch::Tensor A, torch::Tensor B, torch::Tensor C,
                           torch::Tensor state, c10::optional<torch::Tensor> D);
std::vector<int64_t> symm_ipc_handle(torch::Tensor buf);
int64_t symm_open_handle(std::vector<int64_t> bytes);
void symm_close_handle(int64_t ptr);
void symm_allreduce(std::vector<int64_t> peer_ptrs, int64_t payload_bytes,
                    torch::Tensor local_in, torch::Tensor out, int64_t rank,
                    int64_t seq);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("w"),
        pybind11::arg("rstd"), pybind11::arg("dres") = pybind11::none());
  m.def("add_rmsnorm_fwd", &add_rmsnorm_fwd);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("rope_fwd", &rope_fwd);
  m.def("rope_bwd", &rope_bwd);
  m.def("qkv_split_rope_fwd", &qkv_split_rope_fwd);
  m.def("qkv_split_rope_bwd", &qkv_split_rope_bwd);
  m.def("multi_tensor_adamw", &multi_tensor_adamw);
  m.def("multi_tensor_l2norm", &multi_tensor_l2norm);
  m.def("wgrad_gemm_accum", &wgrad_gemm_accum);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_varlen_fwd", &attn_varlen_fwd);
  m.def("attn_varlen_bwd", &attn_varlen_bwd);
  m.def("attn_paged_decode", &attn_paged_decode);
  m.def("attn_paged_prefill", &attn_paged_prefill);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("grouped_gemm", &grouped_gemm);
  m.def("grouped_gemm_probe", &grouped_gemm_probe);
  m.def("grouped_gemm_wgrad", &grouped_gemm_wgrad);
  m.def("grouped_gemm_hip", &grouped_gemm_hip);
  m.def("grouped_gemm_hip_wgrad", &grouped_gemm_hip_wgrad);
  m.def("mx_quantize", &mx_quantize);
  m.def("mx_gemm_nt", &mx_gemm_nt);
  m.def("causal_conv1d_fwd", &causal_conv1d_fwd);
  m.def("causal_conv1d_bwd", &causal_conv1d_bwd);
  m.def("ssd_scan_fwd", &ssd_scan_fwd);
  m.def("ssd_step_fwd", &ssd_step_fwd);
  m.def("symm_ipc_handle", &symm_ipc_handle);
  m.def("symm_open_handle", &symm_open_handle);
  m.def("symm_close_handle", &symm_close_handle);
  m.def("symm_allreduce", &symm_allreduce);
}
