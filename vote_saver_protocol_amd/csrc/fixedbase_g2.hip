// G2 instantiation of the generator-side batch exponentiation (see fixedbase_impl.inc)
#include "fixedbase_impl.inc"

namespace vsp {
template int fixed_base_mul<G2>(vsp_ctx *, const Fr *, size_t, void *);
}  // namespace vsp
