// G2 instantiation of the MSM pipeline (see msm_impl.inc)
#define VSP_MSM_GROUP 2
#include "msm_impl.inc"

namespace vsp {
template int msm_precompute<G2>(vsp_ctx *, G2::Point *, size_t, unsigned);
template int msm_table28<G2>(vsp_ctx *, const G2::Point *, size_t, void *, bool);
template int msm_slot_launch<G2>(vsp_ctx *, unsigned, const MsmRequest &);
template int msm_slot_finish<G2>(vsp_ctx *, unsigned, XYZZ<G2::HF> *, unsigned);
template int msm_slot_finish_wait<G2>(vsp_ctx *, unsigned, unsigned, bool *);
template void msm_slot_fold<G2>(vsp_ctx *, unsigned, XYZZ<G2::HF> *);
template int subgroup_check<G2>(vsp_ctx *, const G2::Point *, size_t, uint32_t *, uint8_t *);
template int bases_to_mont<G2>(vsp_ctx *, const void *, G2::Point *, size_t, int, uint32_t *);
}  // namespace vsp
