// sss_hip_wide_tl.hip - the WIDE instantiation (65..128 executors) once more, recording the executor timelines (kernels *_wide_tl,
// launchers sss_wide_tl_launch_*): sss_hip_wide.hip compiled with SSS_TIMELINE, same flags. See sss_hip_sim_tl.hip.
#define SSS_TIMELINE 1
#include "sss_hip_wide.hip"
