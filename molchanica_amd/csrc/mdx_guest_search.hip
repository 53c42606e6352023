// mdx_guest_search.hip - the search kernel of the guest pose search (mdx_search_guests): pose_search<true> of mdx_pose_search_dev.h as a
// plain kernel, as pose_search_kernel in mdx_poses.hip is pose_search<false>, in a module of its own so that the resident kernels stay
// what they were (the header says why).  One workgroup owns a walker: plain stores only, no atomics.
#include "mdx_pose_search_dev.h"

__global__ __launch_bounds__(256) void guest_search_kernel(SearchArgs a, uint32_t r, const PoseRec* __restrict__ prec, const FlexRec* __restrict__ frec) {
    pose_search<true>(a, r, prec, frec);
}

void mdx_launch_guest_search(hipStream_t st, uint32_t n, const SearchArgs& a, uint32_t r, const PoseRec* prec, const FlexRec* frec) {
    hipLaunchKernelGGL(guest_search_kernel, dim3(n), dim3(256), 0, st, a, r, prec, frec);
}
