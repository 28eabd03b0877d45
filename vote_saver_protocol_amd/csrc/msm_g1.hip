// G1 instantiation of the MSM pipeline (see msm_impl.inc)
#define VSP_MSM_GROUP 1
#include "msm_impl.inc"

namespace vsp {
template int msm_precompute<G1>(vsp_ctx *, G1::Point *, size_t, unsigned);
template int msm_table28<G1>(vsp_ctx *, const G1::Point *, size_t, void *, bool);
template int msm_slot_launch<G1>(vsp_ctx *, unsigned, const MsmRequest &);
template int msm_slot_finish<G1>(vsp_ctx *, unsigned, XYZZ<G1::HF> *, unsigned);
template int msm_slot_finish_wait<G1>(vsp_ctx *, unsigned, unsigned, bool *);
template void msm_slot_fold<G1>(vsp_ctx *, unsigned, XYZZ<G1::HF> *);
template int subgroup_check<G1>(vsp_ctx *, const G1::Point *, size_t, uint32_t *, uint8_t *);
template int bases_to_mont<G1>(vsp_ctx *, const void *, G1::Point *, size_t, int, uint32_t *);
}  // namespace vsp
