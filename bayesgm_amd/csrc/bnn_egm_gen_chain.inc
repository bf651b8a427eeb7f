// bnn_egm_gen_chain.inc -- launchers of the Bayesian generator chain (egm_chain_bnn.h), split over translation units so that the
// six instantiations (each ~50 s of hipcc) compile in parallel.  BNN_GEN_CHAIN_PART selects the instantiations of this unit; nb: 16-row
// tiles of the batch.
#include "bgm_host.h"
#include "bnn_egm_kernels.h"

template <int NTL, int NB, bool PAD = false, int T0 = 1>
static int bnn_egm_gen_chain_launch(const BnnEgmArgs &a, int lds, const EcbTab *tab, float *thetaT, hipStream_t stream) {
  return bgm_launch(bnn_egm_gen_chain_kernel<NTL, NB, PAD, T0>, 1, EGM_THREADS / 64, lds, stream, a, tab, thetaT);
}
#if BNN_GEN_CHAIN_PART == 0
// exact 13-tile extents (p in (191, 207]): B = 32 and B = 16
int bnn_egm_gen_chain_launch_a(const BnnEgmArgs &a, int nb, int lds, const EcbTab *tab, float *thetaT, hipStream_t stream) {
  return nb == 2 ? bnn_egm_gen_chain_launch<13, 2>(a, lds, tab, thetaT, stream) : bnn_egm_gen_chain_launch<13, 1>(a, lds, tab, thetaT, stream);
}
#elif BNN_GEN_CHAIN_PART == 1
// exact 7-tile extents (p in (95, 111])
int bnn_egm_gen_chain_launch_b(const BnnEgmArgs &a, int nb, int lds, const EcbTab *tab, float *thetaT, hipStream_t stream) {
  return nb == 2 ? bnn_egm_gen_chain_launch<7, 2>(a, lds, tab, thetaT, stream) : bnn_egm_gen_chain_launch<7, 1>(a, lds, tab, thetaT, stream);
}
#elif BNN_GEN_CHAIN_PART == 3
// two latent input tiles (16 < q <= 32): the masked 13-tile kernel (B = 32)
int bnn_egm_gen_chain_launch_d(const BnnEgmArgs &a, int, int lds, const EcbTab *tab, float *thetaT, hipStream_t stream) {
  return bnn_egm_gen_chain_launch<13, 2, true, 2>(a, lds, tab, thetaT, stream);
}
#else
// any narrower panel: the 13-tile kernel with masked columns (B = 32)
int bnn_egm_gen_chain_launch_c(const BnnEgmArgs &a, int, int lds, const EcbTab *tab, float *thetaT, hipStream_t stream) {
  return bnn_egm_gen_chain_launch<13, 2, true>(a, lds, tab, thetaT, stream);
}
#endif
