/* td_diag_retained.h -- the measurement hook of the per-launch kernel choice.  Like the hooks
 * of td_diag.h it is NOT part of the drop-in surface (include/tdstep.h) and a
 * production binding should not bind it.  It stands in a header of its own because the host
 * tests hold td_diag.h to exactly its four hooks. */
#ifndef TD_DIAG_RETAINED_H_
#define TD_DIAG_RETAINED_H_

#include "tdstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The step kernel of skipping launches only: a td_step into the retained buffer that leaves
 * clean windows unwritten (td_retain_obs).  kind: enum td_step_kernel_kind.  TD_KERNEL_AUTO
 * gives the kind back to the rule (td_retained_step_kernel's comment in tdstep.h), applied to
 * the kind of a launch that writes every window as it stands; any other kind forces skipping
 * launches and leaves td_step_kernel as it is.  td_set_step_kernel (td_diag.h) overrides it:
 * a kind forced there is forced for every launch, and TD_KERNEL_AUTO there gives both kinds
 * back to their rules.  The three kernels give the same results on the same board state, so
 * any pair is valid (tests/test_gpu_retained_kernel.py).  Fails (and changes nothing) for a
 * small kernel at an L without one.  Synchronises the device. */
int td_set_retained_step_kernel(td_handle* h, int kind);

#ifdef __cplusplus
}
#endif
#endif /* TD_DIAG_RETAINED_H_ */
