// sss_hip_sim_tl.hip - the simulator kernels for up to 64 executors once more, as the instantiation that records the executor
// timelines (sss_sim.h tl_append; kernels *_tl, launchers sss_narrow_tl_launch_*): sss_hip_sim.hip compiled with SSS_TIMELINE, same
// flags. A unit of its own so that the kernels without recording stay exactly the code they were.
#define SSS_TIMELINE 1
#include "sss_hip_sim.hip"
