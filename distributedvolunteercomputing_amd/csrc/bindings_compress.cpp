// Torch bindings for the gradient-compression kernels (kernels/compress.hip).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "kernels/vcx_api_compress.h"

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

#define CHK(x)                                                  \
  TORCH_CHECK((x).is_cuda(), #x " must be a GPU tensor");       \
  TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")

// state: int32[8] on device, prepared by the caller: {0, k, 0, ...}; hist: int32[topk_hist_words()]
// zeros (left zeroed); idx_out / val_out zeroed by the caller (unfilled slots must read 0)
void topk_ef(at::Tensor g, at::Tensor e, int64_t k, at::Tensor state, at::Tensor hist, at::Tensor idx_out,
             at::Tensor val_out) {
  CHK(g);
  CHK(e);
  CHK(state);
  CHK(hist);
  CHK(idx_out);
  CHK(val_out);
  TORCH_CHECK(e.scalar_type() == at::kFloat && g.numel() == e.numel());
  TORCH_CHECK(g.scalar_type() == at::kBFloat16 || g.scalar_type() == at::kFloat);
  TORCH_CHECK(state.scalar_type() == at::kInt && state.numel() >= 8 && hist.scalar_type() == at::kInt &&
              hist.numel() >= vcx_topk_hist_words());
  TORCH_CHECK((reinterpret_cast<uintptr_t>(state.data_ptr()) & 7) == 0, "state must be 8-byte aligned");
  TORCH_CHECK(idx_out.scalar_type() == at::kInt && idx_out.numel() >= k && val_out.numel() >= k);
  TORCH_CHECK(val_out.scalar_type() == at::kBFloat16 || val_out.scalar_type() == at::kFloat);
  TORCH_CHECK(k > 0 && k <= g.numel() && g.numel() < INT32_MAX);
  vcx_topk_ef(g.data_ptr(), g.scalar_type() == at::kBFloat16, e.data_ptr<float>(), g.numel(), (int)k,
              state.data_ptr<int>(), (uint32_t*)hist.data_ptr<int>(), idx_out.data_ptr<int32_t>(), val_out.data_ptr(),
              val_out.scalar_type() == at::kBFloat16, cur_stream());
}

// indices come from other peers: out-of-range ones are dropped inside the kernel (no host sync)
void scatter_add(at::Tensor idx, at::Tensor val, double scale, at::Tensor dense) {
  CHK(idx);
  CHK(val);
  CHK(dense);
  TORCH_CHECK(idx.scalar_type() == at::kInt && dense.scalar_type() == at::kFloat && idx.numel() == val.numel());
  TORCH_CHECK(val.scalar_type() == at::kBFloat16 || val.scalar_type() == at::kFloat);
  TORCH_CHECK(dense.numel() < INT32_MAX);
  vcx_scatter_add(idx.data_ptr<int32_t>(), val.data_ptr(), val.scalar_type() == at::kBFloat16, idx.numel(),
                  (float)scale, dense.data_ptr<float>(), dense.numel(), cur_stream());
}

// wire: int32 [P, L]; per peer k indices then k values of `val_dtype` (bf16 or fp32) packed after them
void scatter_add_packed(at::Tensor wire, int64_t k, bool val_bf16, double scale, at::Tensor dense) {
  CHK(wire);
  CHK(dense);
  TORCH_CHECK(wire.scalar_type() == at::kInt && wire.dim() == 2 && dense.scalar_type() == at::kFloat);
  const int64_t L = wire.size(1), vw = val_bf16 ? (k + 1) / 2 : k;
  TORCH_CHECK(k > 0 && L >= k + vw, "scatter_add_packed: wire rows too short for k pairs");
  TORCH_CHECK(dense.numel() < INT32_MAX && wire.size(0) * k < INT32_MAX);
  vcx_scatter_add_packed(wire.data_ptr<int32_t>(), (int)wire.size(0), (int)k, L, val_bf16, (float)scale,
                         dense.data_ptr<float>(), dense.numel(), cur_stream());
}

int64_t topk_hist_words() { return vcx_topk_hist_words(); }

void check_desc(const at::Tensor& d, int64_t nmat) {
  CHK(d);
  TORCH_CHECK(d.scalar_type() == at::kByte && d.numel() == nmat * vcx_psgd_desc_size(), "bad descriptor table");
}

// M += G (error feedback, skipped when G is None) fused with P = M Q over every matrix; lazy: the
// previous reconstruct ran with update_m=false, so M -= P_prev Q^T is applied first
void psgd_mq(at::Tensor desc, int64_t nmat, int64_t nblocks, at::Tensor M, at::Tensor Q, at::Tensor P, int64_t rank,
             std::optional<at::Tensor> G, bool lazy) {
  check_desc(desc, nmat);
  CHK(M);
  CHK(Q);
  CHK(P);
  const void* g = nullptr;
  if (G.has_value()) {
    CHK((*G));
    TORCH_CHECK(G->scalar_type() == at::kBFloat16 && G->numel() == M.numel(), "psgd_mq: G must be bf16 like M");
    g = G->data_ptr();
  }
  vcx_psgd_mq(desc.data_ptr(), (int)nmat, (int)nblocks, M.data_ptr<float>(), g, Q.data_ptr<float>(),
              P.data_ptr<float>(), (int)rank, lazy ? 1 : 0, cur_stream());
}

void psgd_mtp(at::Tensor desc, int64_t nmat, int64_t nblocks, at::Tensor M, at::Tensor P, at::Tensor Q, int64_t rank) {
  check_desc(desc, nmat);
  CHK(M);
  CHK(Q);
  CHK(P);
  vcx_psgd_mtp(desc.data_ptr(), (int)nmat, (int)nblocks, M.data_ptr<float>(), P.data_ptr<float>(),
               Q.data_ptr<float>(), (int)rank, cur_stream());
}

void psgd_orth(at::Tensor desc, int64_t nmat, int64_t nblocks, at::Tensor P, at::Tensor G, int64_t rank) {
  check_desc(desc, nmat);
  CHK(P);
  CHK(G);
  TORCH_CHECK(P.scalar_type() == at::kFloat && G.scalar_type() == at::kFloat && G.numel() >= 2 * nmat * rank * rank,
              "psgd_orth: G must hold 2 * nmat * rank^2 floats");
  vcx_psgd_orth(desc.data_ptr(), (int)nmat, (int)nblocks, P.data_ptr<float>(), G.data_ptr<float>(), (int)rank,
                cur_stream());
}

void psgd_reconstruct(at::Tensor desc, int64_t nmat, int64_t nblocks, at::Tensor M, at::Tensor P, at::Tensor Q,
                      at::Tensor out, int64_t rank, bool update_m) {
  check_desc(desc, nmat);
  CHK(M);
  CHK(P);
  CHK(Q);
  CHK(out);
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 && out.numel() == M.numel());
  vcx_psgd_reconstruct(desc.data_ptr(), (int)nmat, (int)nblocks, M.data_ptr<float>(), P.data_ptr<float>(),
                       Q.data_ptr<float>(), out.data_ptr(), (int)rank, update_m ? 1 : 0, cur_stream());
}

void ef_accum(at::Tensor g, at::Tensor e) {
  CHK(g);
  CHK(e);
  TORCH_CHECK(g.scalar_type() == at::kBFloat16 && e.scalar_type() == at::kFloat && g.numel() == e.numel() &&
              g.numel() % 8 == 0);
  vcx_ef_accum(g.data_ptr(), e.data_ptr<float>(), g.numel(), cur_stream());
}

// q8 layout of n elements over P peers: L = P m padded elements, m a multiple of the block, and no
// more padding than one block per peer; a buffer of records holds L codes + L / 32 bytes of scales
void check_q8(int64_t n, int64_t L, int64_t P, const at::Tensor& records, const char* what) {
  const int64_t B = vcx_q8_block();
  TORCH_CHECK(n > 0 && n < INT32_MAX && P >= 1 && L % (B * P) == 0 && L >= n && L - n < B * P && L < (1ll << 34),
              what, ": bad layout n=", n, " L=", L, " P=", P);
  TORCH_CHECK(records.scalar_type() == at::kByte && records.numel() >= L + L / 32, what, ": record buffer too short");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(records.data_ptr()) & 15) == 0, what, ": records must be 16-byte aligned");
}

// v = e + g encoded into the P records of `wire`; e keeps v - decoded. g: bf16 or fp32 [n], e: fp32 [n]
void q8_encode(at::Tensor g, at::Tensor e, int64_t L, int64_t P, at::Tensor wire) {
  CHK(g);
  CHK(e);
  CHK(wire);
  TORCH_CHECK(e.scalar_type() == at::kFloat && g.numel() == e.numel());
  TORCH_CHECK(g.scalar_type() == at::kBFloat16 || g.scalar_type() == at::kFloat);
  check_q8(g.numel(), L, P, wire, "q8_encode");
  vcx_q8_encode(g.data_ptr(), g.scalar_type() == at::kBFloat16, e.data_ptr<float>(), g.numel(), L, (int)P,
                wire.data_ptr<uint8_t>(), cur_stream());
}

// recv: P records of a shard of m elements (the peers in rank order); out_record: one record of
// avg_scale * their sum
void q8_reduce(at::Tensor recv, int64_t P, int64_t m, double avg_scale, at::Tensor out_record) {
  CHK(recv);
  CHK(out_record);
  check_q8(m, m, 1, out_record, "q8_reduce");
  TORCH_CHECK(P >= 1 && P <= INT32_MAX && recv.scalar_type() == at::kByte && recv.numel() >= P * (m + m / 32),
              "q8_reduce: recv must hold P records");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(recv.data_ptr()) & 15) == 0, "q8_reduce: recv must be 16-byte aligned");
  vcx_q8_reduce(recv.data_ptr<uint8_t>(), (int)P, m, (float)avg_scale, out_record.data_ptr<uint8_t>(), cur_stream());
}

// The robust sibling of q8_reduce: out_record = one record of the trimmed mean (ops/robust.py) over the rows of
// live_mask; elements at or beyond `valid` do not vote. counts: int64 [P], nonfinite: int64 [1], both optional.
// Everything is checked here, before the launcher's own checks, so a refused call leaves every output unwritten.
void q8_trimmed_reduce(at::Tensor recv, int64_t P, int64_t m, int64_t trim, int64_t live_mask, int64_t valid,
                       at::Tensor out_record, std::optional<at::Tensor> counts, std::optional<at::Tensor> nonfinite) {
  CHK(recv);
  CHK(out_record);
  TORCH_CHECK(P >= 1 && P <= 16, "q8_trimmed_reduce: P must be in 1..16, got ", P);
  TORCH_CHECK(live_mask > 0 && (live_mask >> P) == 0,
              "q8_trimmed_reduce: live_mask must name at least one of the P rows and no other, got ", live_mask);
  TORCH_CHECK(trim >= 0, "q8_trimmed_reduce: trim must be >= 0");
  check_q8(m, m, 1, out_record, "q8_trimmed_reduce");
  TORCH_CHECK(valid >= 0 && valid <= m, "q8_trimmed_reduce: valid must be in 0..m, got ", valid);
  TORCH_CHECK(recv.scalar_type() == at::kByte && recv.numel() >= P * (m + m / 32),
              "q8_trimmed_reduce: recv must hold P records");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(recv.data_ptr()) & 15) == 0,
              "q8_trimmed_reduce: recv must be 16-byte aligned");
  TORCH_CHECK(out_record.get_device() == recv.get_device(), "q8_trimmed_reduce: out_record must be on recv's device");
  auto counter = [&](const std::optional<at::Tensor>& t, int64_t len, const char* what) -> int64_t* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->is_cuda() && t->get_device() == recv.get_device() && t->numel() == len && t->is_contiguous() &&
                    t->scalar_type() == at::kLong,
                "q8_trimmed_reduce: ", what, " must hold ", len, " int64 on recv's device");
    return t->data_ptr<int64_t>();
  };
  int64_t* c = counter(counts, P, "counts");
  int64_t* nf = counter(nonfinite, 1, "nonfinite");
  vcx_q8_trimmed_reduce(recv.data_ptr<uint8_t>(), (int)P, m, (int)std::min<int64_t>(trim, 16), (uint32_t)live_mask,
                        valid, out_record.data_ptr<uint8_t>(), c, nf, cur_stream());
}

// Centered clipping over the q8 records (the cclip sibling of q8_trimmed_reduce): out_record = one record of the rule
// of ops/robust.py over the decoded rows of live_mask, `iters` updates with radius tau (0: adaptive); elements at or
// beyond `valid` do not vote. weights: fp32 [P], nonfinite: int64 [1], both optional. The workspace (the fp32 centre,
// the distances' chunk partials, the weights) is allocated here. Everything is checked before the launcher's own
// checks, so a refused call leaves every output unwritten.
void q8_cclip_reduce(at::Tensor recv, int64_t P, int64_t m, int64_t live_mask, int64_t valid, double tau, int64_t iters,
                     at::Tensor out_record, std::optional<at::Tensor> weights, std::optional<at::Tensor> nonfinite) {
  CHK(recv);
  CHK(out_record);
  TORCH_CHECK(P >= 1 && P <= 16, "q8_cclip_reduce: P must be in 1..16, got ", P);
  TORCH_CHECK(live_mask > 0 && (live_mask >> P) == 0,
              "q8_cclip_reduce: live_mask must name at least one of the P rows and no other, got ", live_mask);
  TORCH_CHECK(tau >= 0.0 && tau <= 3.4028234663852886e38,  // a finite fp32 value; a NaN fails both comparisons
              "q8_cclip_reduce: tau must be finite and >= 0 (0: adaptive), got ", tau);
  TORCH_CHECK(iters >= 1 && iters <= 8, "q8_cclip_reduce: iters must be in 1..8, got ", iters);
  check_q8(m, m, 1, out_record, "q8_cclip_reduce");
  TORCH_CHECK(valid >= 0 && valid <= m, "q8_cclip_reduce: valid must be in 0..m, got ", valid);
  TORCH_CHECK(recv.scalar_type() == at::kByte && recv.numel() >= P * (m + m / 32),
              "q8_cclip_reduce: recv must hold P records");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(recv.data_ptr()) & 15) == 0, "q8_cclip_reduce: recv must be 16-byte aligned");
  TORCH_CHECK(out_record.get_device() == recv.get_device(), "q8_cclip_reduce: out_record must be on recv's device");
  if (weights)
    TORCH_CHECK(weights->is_cuda() && weights->get_device() == recv.get_device() && weights->numel() == P &&
                    weights->is_contiguous() && weights->scalar_type() == at::kFloat,
                "q8_cclip_reduce: weights must hold P fp32 on recv's device");
  if (nonfinite)
    TORCH_CHECK(nonfinite->is_cuda() && nonfinite->get_device() == recv.get_device() && nonfinite->numel() == 1 &&
                    nonfinite->is_contiguous() && nonfinite->scalar_type() == at::kLong,
                "q8_cclip_reduce: nonfinite must hold 1 int64 on recv's device");
  at::Tensor ws = at::empty({vcx_q8_cclip_workspace_floats((int)P, m)}, recv.options().dtype(at::kFloat));
  vcx_q8_cclip_reduce(recv.data_ptr<uint8_t>(), (int)P, m, (uint32_t)live_mask, valid, (float)tau, (int)iters,
                      out_record.data_ptr<uint8_t>(), weights ? weights->data_ptr<float>() : nullptr,
                      nonfinite ? nonfinite->data_ptr<int64_t>() : nullptr, ws.data_ptr<float>(), cur_stream());
}

// records: P records covering L elements; out: bf16 [n], the first n decoded values
void q8_decode(at::Tensor records, int64_t L, int64_t P, at::Tensor out) {
  CHK(records);
  CHK(out);
  TORCH_CHECK(out.scalar_type() == at::kBFloat16);
  check_q8(out.numel(), L, P, records, "q8_decode");
  vcx_q8_decode(records.data_ptr<uint8_t>(), out.numel(), L, (int)P, out.data_ptr(), cur_stream());
}

}  // namespace

void vcx_register_compress(pybind11::module& m) {
  m.def("q8_encode", &q8_encode);
  m.def("q8_reduce", &q8_reduce);
  m.def("q8_decode", &q8_decode);
  m.def("q8_trimmed_reduce", &q8_trimmed_reduce, pybind11::arg("recv"), pybind11::arg("P"), pybind11::arg("m"),
        pybind11::arg("trim"), pybind11::arg("live_mask"), pybind11::arg("valid"), pybind11::arg("out_record"),
        pybind11::arg("counts") = pybind11::none(), pybind11::arg("nonfinite") = pybind11::none());
  m.def("q8_trimmed_reduce_max_blocks", &vcx_q8_trimmed_reduce_max_blocks);
  m.def("q8_cclip_reduce", &q8_cclip_reduce, pybind11::arg("recv"), pybind11::arg("P"), pybind11::arg("m"),
        pybind11::arg("live_mask"), pybind11::arg("valid"), pybind11::arg("tau"), pybind11::arg("iters"),
        pybind11::arg("out_record"), pybind11::arg("weights") = pybind11::none(),
        pybind11::arg("nonfinite") = pybind11::none());
  m.def("q8_cclip_max_workgroups", &vcx_q8_cclip_max_workgroups);
  m.def("q8_block", &vcx_q8_block);
  m.def("topk_ef", &topk_ef);
  m.def("scatter_add", &scatter_add);
  m.def("scatter_add_packed", &scatter_add_packed);
  m.def("topk_hist_words", &topk_hist_words);
  m.def("psgd_mq", &psgd_mq, pybind11::arg("desc"), pybind11::arg("nmat"), pybind11::arg("nblocks"),
        pybind11::arg("M"), pybind11::arg("Q"), pybind11::arg("P"), pybind11::arg("rank"),
        pybind11::arg("G") = pybind11::none(), pybind11::arg("lazy") = false);
  m.def("psgd_mtp", &psgd_mtp);
  m.def("psgd_orth", &psgd_orth);
  m.def("psgd_orth_rows", &vcx_psgd_orth_rows);
  m.def("psgd_reconstruct", &psgd_reconstruct, pybind11::arg("desc"), pybind11::arg("nmat"), pybind11::arg("nblocks"),
        pybind11::arg("M"), pybind11::arg("P"), pybind11::arg("Q"), pybind11::arg("out"), pybind11::arg("rank"),
        pybind11::arg("update_m") = true);
  m.def("ef_accum", &ef_accum);
  m.def("psgd_desc_size", &vcx_psgd_desc_size);
  m.def("psgd_rows_per_block", &vcx_psgd_rows_per_block);
  m.def("psgd_mtp_rows", &vcx_psgd_mtp_rows);
  m.def("psgd_mtp_cols", &vcx_psgd_mtp_cols);
}
