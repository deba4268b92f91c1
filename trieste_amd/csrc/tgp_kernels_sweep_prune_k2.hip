// fused EI arg-max sweep with candidate-block pruning, kernel kind 2: sweep_dma_kernel<KIND, DP, PRUNE = true>
// (tgp_kernels_sweep_dma.inc), in a translation unit of its own so that the plain instantiations keep their code
#define TGP_SWEEP_KIND 2
#define TGP_SWEEP_PRUNE_TU 1
#include "tgp_kernels_sweep_dma.inc"
