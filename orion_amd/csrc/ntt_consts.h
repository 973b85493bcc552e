// NTT launch constants shared by the kernels (common.h) and the host-only
// launch planner (ntt_route.h): plain integers, no HIP types
#pragma once

// NTT launch prologues and epilogues (the launch descriptor: common.h NttIO)
enum { NTT_PRO_LOAD = 0, NTT_PRO_RESCALE = 2, NTT_PRO_BEXT = 3 };
// NTT_EPI_SUBSCALE_AUT: the subtract-and-scale epilogue storing element e at
// position aut[e] -- the NTT-domain automorphism of a rotation (its scatter
// index, the gather index of the inverse Galois element) applied in the
// ModDown's store instead of by a separate automorph launch
// NTT_EPI_SUBSCALE_AUT_ACC: the same, added to the word already at aut[e] (a
// rotation whose result is added to its own input, x += sigma_g(x))
enum { NTT_EPI_STORE = 0, NTT_EPI_SUBSCALE = 1, NTT_EPI_SUBSCALE_AUT = 2, NTT_EPI_SUBSCALE_AUT_ACC = 3 };
