// mdx_guest_flex.hip - the flexible step kernel of the guest refinement (mdx_refine_guests_flex): pose_step<true, true> of
// mdx_pose_step_dev.h as a plain kernel, as its three siblings in mdx_poses.hip are, in a module of its own so that theirs stays
// what it was (the header says why).  One workgroup owns a pose: plain stores only, no atomics.
#include "mdx_pose_step_dev.h"

__global__ __launch_bounds__(256) void guest_flex_step_kernel(StepArgs a) { pose_step<true, true>(a); }

void mdx_launch_guest_flex_step(hipStream_t st, uint32_t n, const StepArgs& a) {
    hipLaunchKernelGGL(guest_flex_step_kernel, dim3(n), dim3(256), 0, st, a);
}
