// Flushes a KernelBatch: every queue of a scheduling round goes out as grouped
// launches, critical-path kernels first, under the batch's launch settings.
#include <algorithm>

#include "kernels.hpp"
#include "launch_settings.hpp"

namespace parsec {

namespace kern {
LaunchSettings& launch_settings() {
  static thread_local LaunchSettings s;
  return s;
}
}  // namespace kern

size_t kernel_batch_workspace_bytes(const KernelBatch& b) {
  size_t w = 0;
  for (auto& p : b.potrf) w = std::max(w, kern::potrf_steps_eligible(p) ? kern::potrf_steps_workspace_bytes(p) : kern::potrf_workspace_bytes(p));
  for (auto& g : b.getrf) w = std::max(w, kern::getrf_workspace_bytes(g));
  if (!b.lu_panel.empty()) w = std::max(w, kern::lu_panel_workspace_bytes());
  for (auto& t : b.trtri) w = std::max(w, kern::trtri_workspace_bytes(t));
  for (auto& l : b.lauum) w = std::max(w, kern::lauum_workspace_bytes(l));
  if (!b.trsm_w.empty()) w = std::max(w, kern::trsm_w_workspace_bytes(b.trsm_w.data(), (int)b.trsm_w.size()));
  if (!b.qr_panel.empty()) w = std::max(w, kern::qr_panel_workspace_bytes(b.qr_panel.data(), (int)b.qr_panel.size()));
  w = std::max(w, kern::trsm_workspace_bytes(b.trsm.data(), (int)b.trsm.size()));
  w = std::max(w, kern::trsm_left_workspace_bytes(b.trsm_left.data(), (int)b.trsm_left.size()));
  return std::max(w, kern::qr_apply_workspace_bytes(b.qr_apply.data(), (int)b.qr_apply.size()));
}

void launch_kernel_batch(KernelBatch& b, hipStream_t stream, void* ws) {
  const kern::LaunchScope scope({b.critical ? 1 : 0, b.one_per_cu ? kern::kBulkPadBytes : 0, b.claim_cus, b.bulk_yield ? 1 : 0});
  // critical-path kernels first: a POTRF's fused update, POTRF, then TRSM, then the GEMM/SYRK updates
  if (!b.pre_gemm.empty()) kern::launch_gemm_batch(b.pre_gemm.data(), (int)b.pre_gemm.size(), stream);
  for (auto& p : b.potrf) {
    if (kern::potrf_steps_eligible(p)) kern::launch_potrf_steps(p, stream, static_cast<double*>(ws));
    else kern::launch_potrf(p, stream, static_cast<double*>(ws));
  }
  for (auto& g : b.getrf) kern::launch_getrf_nopiv(g, stream, static_cast<double*>(ws));
  for (auto& g : b.lu_panel) kern::launch_lu_panel(g, stream, static_cast<double*>(ws));
  if (!b.qr_panel.empty()) kern::launch_qr_panel_blocked(b.qr_panel.data(), (int)b.qr_panel.size(), stream, static_cast<double*>(ws));
  if (!b.trsm.empty()) kern::launch_trsm_batch(b.trsm.data(), (int)b.trsm.size(), stream, static_cast<double*>(ws));
  if (!b.trsm_w.empty()) kern::launch_trsm_w_batch(b.trsm_w.data(), (int)b.trsm_w.size(), stream, static_cast<double*>(ws));
  // GESSM / SSSSM: the interchanges, then the unit lower solves; their updates are GEMMs
  if (!b.laswp.empty()) kern::launch_laswp_batch(b.laswp.data(), (int)b.laswp.size(), stream);
  if (!b.trsm_left.empty()) kern::launch_trsm_left_batch(b.trsm_left.data(), (int)b.trsm_left.size(), stream, static_cast<double*>(ws));
  if (!b.qr_apply.empty()) kern::launch_qr_apply(b.qr_apply.data(), (int)b.qr_apply.size(), stream, static_cast<double*>(ws));
  // the inverse kernels (DTRTRI / DLAUUM): a round's TRMMs are one grouped launch
  for (auto& t : b.trtri) kern::launch_trtri(t, stream, static_cast<double*>(ws));
  if (!b.trmm.empty()) kern::launch_trmm_lt_batch(b.trmm.data(), (int)b.trmm.size(), stream);
  for (auto& l : b.lauum) kern::launch_lauum(l, stream, static_cast<double*>(ws));
  if (!b.gemm.empty()) kern::launch_gemm_batch(b.gemm.data(), (int)b.gemm.size(), stream);
  if (!b.stencil.empty()) kern::launch_stencil7_batch(b.stencil.data(), (int)b.stencil.size(), stream);
  for (auto& g : b.generic) g(stream);
}

}  // namespace parsec
