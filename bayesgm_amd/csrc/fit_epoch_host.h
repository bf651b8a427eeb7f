// fit_epoch_host.h -- what the in-library epoch loops (bgm_causal_fit_epoch in fit_api.hip, bgm_bnn_fit_epoch in bnn_api.hip) share on
// the host: the handle's second stream and its events, the device counters of fit_sync.h with the probe that allows them, and the
// check that reports a device-side wait that gave up.  Host only: the probe's two kernels live in fit_sync.h.
#pragma once
#include <string>

#include "bgm_host.h"
#include "fit_launch.h"
#include "fit_sync.h"

// a device-side wait of the previous epoch call `who` gave up (fit_sync.h): that call's results are void
static inline int epoch_check(bgm_handle *h, hipStream_t stream, const char *who) {
  if (!h->epoch_ctr) return BGM_OK;
  unsigned c[4];
  BGM_HIP_CHECK(hipMemcpyAsync(c, h->epoch_ctr, sizeof(c), hipMemcpyDeviceToHost, stream));
  BGM_HIP_CHECK(hipStreamSynchronize(stream));
  if (!c[2]) return BGM_OK;
  BGM_HIP_CHECK(hipMemset(h->epoch_ctr, 0, sizeof(c)));
  h->epoch_theta_done = h->epoch_z_done = 0;
  bgm_set_error(std::string(who) + ": a device-side ordering wait timed out in the previous call (its updates are unordered); "
                "BGM_FIT_NO_FLAGS=1 orders the two streams with HIP events instead");
  return BGM_E_HIP;
}

// the handle's second stream and one event pair per minibatch in flight, created at the first call that overlaps its phases
static inline int epoch_streams_begin(bgm_handle *h) {
  if (h->epoch_stream) return BGM_OK;
  BGM_HIP_CHECK(hipStreamCreateWithFlags(&h->epoch_stream, hipStreamNonBlocking));
  for (int k = 0; k < 4; ++k) {
    BGM_HIP_CHECK(hipEventCreateWithFlags(&h->epoch_ev_t[k], hipEventDisableTiming));
    BGM_HIP_CHECK(hipEventCreateWithFlags(&h->epoch_ev_z[k], hipEventDisableTiming));
  }
  return BGM_OK;
}

// The device counters of a call that wants them: allocated and zeroed at the first one, checked for a wait the previous call gave up
// on at every later one.  *usable: the two streams run side by side -- probed once per handle and caller stream (fit_sync_probe); where
// they do not (a profiler serialising kernels, one hardware queue) the caller orders them with HIP events.
static inline int epoch_flags_begin(bgm_handle *h, hipStream_t sA, hipStream_t sB, const char *who, bool *usable) {
  if (!h->epoch_ctr) {
    BGM_HIP_CHECK(hipMalloc((void **)&h->epoch_ctr, sizeof(unsigned) * 8));
    BGM_HIP_CHECK(hipMemsetAsync(h->epoch_ctr, 0, sizeof(unsigned) * 8, sA));
    h->epoch_theta_done = h->epoch_z_done = 0;
  } else if (int rc = epoch_check(h, sA, who)) return rc;
  if (!h->epoch_flags_ok || h->epoch_probe_stream != (void *)sA) {
    int ok = 0;
    BGM_HIP_CHECK(fit_sync_probe(sA, sB, h->epoch_ctr + 4, &ok));
    h->epoch_flags_ok = ok ? 1 : -1;
    h->epoch_probe_stream = (void *)sA;
  }
  *usable = h->epoch_flags_ok > 0;
  return BGM_OK;
}
