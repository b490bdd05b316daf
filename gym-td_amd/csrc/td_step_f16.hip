// td_step_f16.hip -- the step kernels that write a float16 observation (td_set_obs_format),
// as a compilation unit of their own: td_step.hip with only launch_step_f16 and the
// kernels it launches (see there).
#define TD_STEP_F16_UNIT 1
#include "td_step.hip"
