"""CausalBGM -- host-side mirror of the reference class (same constructor, method
names, argument meaning, return values, error behaviour and output files), driving the
gfx950 kernels of libbgm_hip.so.

Mirrors /root/reference/src/bayesgm/models/causalbgm/base.py:
    __init__ :56-128   get_config :130   fit :434   evaluate :535   predict :573
    metropolis_hastings_sampler :820   infer_from_latent_posterior :672
This class holds the deterministic networks (``use_bnn=False``); with ``use_bnn=True`` (the
reference's default) the constructor returns the Bayesian-network subclass of causalbgm_bnn.py.
"""
import datetime
import os
from statistics import NormalDist

import numpy as np
import torch

# Default BatchNormalization reading of the layers the reference calls without `training=` (Discriminator, networks/base.py:378;
# BayesianFullyConnectedNet, networks/bnn.py:26): inference mode.  This is the reading under which the build reproduces the
# training log, acceptance rate and ADRF error the reference published (tests/golden/tutorial_trace.json, DESIGN_HISTORY.md section 2b);
# "batch" (batch statistics, what Keras 2.10's documented training-mode propagation implies for the code as written) stays
# available as params['disc_norm'] / params['bnn_norm'] = "batch".
DISC_NORM_DEFAULT = "fixed"
BNN_NORM_DEFAULT = "fixed"

from .. import _lib, diagnostics, host_rng, parallel
from .. import row_adapt as row_adapt_mod
from .. import causal_hmc as hmc_mod
from ..engine import CausalEngine
from ..datasets import Gaussian_sampler
from ..utils import save_data
from ._checkpoint import CheckpointManager

_DEFAULTS = dict(use_bnn=True, g_units=[64] * 5, e_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
                 dz_units=[64, 32, 8], lr=0.0002, lr_theta=0.0001, lr_z=0.0001, g_d_freq=5, save_model=False,
                 save_res=True, kl_weight=0.0001, use_z_rec=True)


def _glorot(rs, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rs.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


def _init_mlp(rs, dims):
    """Keras Dense defaults: glorot-uniform kernel, zero bias (networks/base.py:17-26)."""
    return [(_glorot(rs, dims[i], dims[i + 1]), np.zeros(dims[i + 1], np.float32)) for i in range(len(dims) - 1)]


def _disc_norm(p):
    """params['disc_norm'] (build option): BatchNormalization mode of the EGM discriminators, "batch" | "fixed"
    (include/bgm_hip.h bgm_set_disc_norm, DESIGN_HISTORY.md section 2b)."""
    mode = p.get("disc_norm", DISC_NORM_DEFAULT)
    if mode not in ("batch", "fixed"):
        raise ValueError("params['disc_norm'] must be 'batch' or 'fixed'")
    if "disc_norm" not in p and mode != "batch":      # a default that is not the reference as written: said once per process
        diagnostics.notice_once("disc_norm", "params['disc_norm'] not given: the EGM discriminators normalise in inference mode ('fixed'); "
                                "'batch' runs their BatchNormalization on batch statistics as networks/base.py:364-379 reads (DESIGN_HISTORY.md section 2b)")
    return mode


class CausalBGM(object):
    mcmc_diagnostics_ = None         # diagnostics.ChainDiagnostics of the last sampler call that asked for them
    hmc_row_leapfrog_ = None         # mean leapfrog steps per retained transition of every row (NumPy [n]) of the last HMC call with max_trajectory / jitter_leapfrog; None without
    hmc_row_step_ = None             # per-row HMC step sizes (NumPy, global row order) of the last predict(sampler='hmc') / hmc_sampler call
    hmc_row_mass_ = None             # per-row, per-coordinate HMC metric scales [n, q] (NumPy, global row order) of the last mass='diag' call; None otherwise
    individual_sd_ = None            # per-row, per-dose posterior sd [n, n_doses] (NumPy float64) of the last predict_individual call
    group_dose_response_ = None      # {label: (mean [n_doses], sd [n_doses])} of the last predict_individual(groups=...) call; None otherwise
    mh_row_scale_ = None             # per-row proposal scales (NumPy, global row order) of the last predict / sampler call; None when it ran without row adaptation

    def __new__(cls, params, *args, **kwargs):
        # params['use_bnn'] (default True, base.py:64): the Bayesian-network model lives in causalbgm_bnn.py
        if cls is CausalBGM and dict(_DEFAULTS, **params)["use_bnn"]:
            from .causalbgm_bnn import CausalBGMBayes
            return super().__new__(CausalBGMBayes)
        return super().__new__(cls)

    def __init__(self, params, timestamp=None, random_seed=None, device=None):
        self.params = params
        self.timestamp = timestamp
        p = dict(_DEFAULTS)
        p.update(params)
        self._p = p
        random_seed = parallel.shared_seed(random_seed)   # None stays None in a single process; one seed for all ranks otherwise
        self._rs = np.random.RandomState(random_seed) if random_seed is not None else np.random.RandomState()
        if random_seed is not None:
            np.random.seed(random_seed)
        self._seed_counter = 0
        self._base_seed = int(random_seed) if random_seed is not None else int(np.random.randint(0, 2 ** 31 - 1))
        z = list(p["z_dims"])
        q = sum(z)
        self.nets = {
            "g": _init_mlp(self._rs, [q] + list(p["g_units"]) + [p["v_dim"] + 1]),
            "e": _init_mlp(self._rs, [p["v_dim"]] + list(p["e_units"]) + [q]),
            "f": _init_mlp(self._rs, [z[0] + z[1] + 1] + list(p["f_units"]) + [2]),
            "h": _init_mlp(self._rs, [z[0] + z[2]] + list(p["h_units"]) + [2]),
        }
        self.z_sampler = Gaussian_sampler(mean=np.zeros(q), sd=1.0)
        if device is None:
            device = int(os.environ.get("BGM_DEVICE", os.environ.get("LOCAL_RANK", 0)))   # BGM_DEVICE: dev aid
        self.engine = CausalEngine(p["v_dim"], z, binary_treatment=p["binary_treatment"], g_units=p["g_units"],
                                   f_units=p["f_units"], h_units=p["h_units"], e_units=p["e_units"],
                                   sigma_v=params.get("sigma_v"), sigma_x=params.get("sigma_x"),
                                   sigma_y=params.get("sigma_y"), device=device)
        self.engine.set_disc_norm(_disc_norm(p))
        # params['mh_precision'] (build option): arithmetic of the posterior-sampling kernels of predict /
        # metropolis_hastings_sampler / get_log_posterior: "fp32" (default, the reference's arithmetic) or "bf16x3" (split
        # precision on the bf16 matrix pipe, DESIGN_HISTORY.md section 4b)
        if p.get("mh_precision", "fp32") not in ("fp32", "bf16x3", "f16x3"):
            raise ValueError("params['mh_precision'] must be 'fp32', 'bf16x3' or 'f16x3'")
        self.engine.set_precision(p.get("mh_precision", "fp32"))
        # params['outcome_cache'] (build option, default True): predict's ADRF sampler evaluates the outcome net only for the chains that
        # moved since the last retained draw (identical results; 'wave' = per 16-chain tile, the round-4 form; False = evaluate f at
        # every retained draw as the reference).  params['event_budget_mb']: bound on the event buffers of one segment (default 8192).
        self.engine.set_outcome_cache(p.get("outcome_cache", True))
        if p.get("event_budget_mb"):
            self.engine.set_event_budget(int(p["event_budget_mb"]) << 20)
        self._push_weights()
        if self.timestamp is None:
            self.timestamp = datetime.datetime.now().astimezone().strftime('%Y%m%d_%H%M%S')
        self.checkpoint_path = "{}/checkpoints/{}/{}".format(params['output_dir'], params['dataset'], self.timestamp)
        if p['save_model'] and not os.path.exists(self.checkpoint_path):
            os.makedirs(self.checkpoint_path, exist_ok=True)
        self.save_dir = "{}/results/{}/{}".format(params['output_dir'], params['dataset'], self.timestamp)
        if p['save_res'] and not os.path.exists(self.save_dir):
            os.makedirs(self.save_dir, exist_ok=True)
        self.data_z = None
        self.last_acceptance_rate = None
        self._fit_live = None            # (zm, zv) of the running fit, for checkpoints
        self._restored_opt = None        # optimizer slots of a restored checkpoint, installed by the next fit
        self._restore_latest()

    def _restore_latest(self):
        """tf.train.CheckpointManager(..., max_to_keep=5) + restore of the latest checkpoint at construction (base.py:124-128)."""
        self.ckpt_manager = CheckpointManager(self.checkpoint_path, max_to_keep=5)
        latest = self.ckpt_manager.latest_checkpoint
        if latest:
            self.load_checkpoint(latest)
            print('Latest checkpoint restored!!')

    # ------------------------------------------------------------------ plumbing
    def get_config(self):
        return {"params": self.params}

    def _push_weights(self, which=("g", "f", "h", "e")):
        ids = {"g": _lib.NET_G, "f": _lib.NET_F, "h": _lib.NET_H, "e": _lib.NET_E}
        for k in which:
            self.engine.set_weights(ids[k], self.nets[k])

    def set_weights(self, **nets):
        """Install network parameters ([(W, b), ...] per net) -- the counterpart of restoring a checkpoint."""
        for k, v in nets.items():
            self.nets[k] = [(np.asarray(W, np.float32), np.asarray(b, np.float32)) for W, b in v]
        self._push_weights(tuple(nets))

    def _next_seed(self):
        self._seed_counter += 1
        return (self._base_seed * 1000003 + self._seed_counter) & 0x7FFFFFFFFFFFFFFF

    def _dev(self, a):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.engine.device, dtype=torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.engine.device)

    def _panel_v_var(self, v):
        """mean per-column variance of this rank's rows of V (1 for a standardised panel), cached per tensor: diagnostics.py compares
        MSE_v / var(V)"""
        key = (v.data_ptr(), tuple(v.shape))
        if getattr(self, '_v_var_key', None) != key:
            self._v_var_key = key
            self._v_var = float(v.var(dim=0, unbiased=False).mean().item()) if v.shape[0] > 1 else 1.0
        return self._v_var

    # ------------------------------------------------------------------ fit
    def _net_dims(self, k):
        return [self.nets[k][0][0].shape[0]] + [W.shape[1] for W, _ in self.nets[k]]

    def _pull_weights(self, which=("g", "f", "h")):
        ids = {"g": _lib.NET_G, "f": _lib.NET_F, "h": _lib.NET_H, "e": _lib.NET_E}
        for k in which:
            self.nets[k] = self.engine.get_weights(ids[k], self._net_dims(k))

    @staticmethod
    def _choice_no_replace(n, k):
        """np.random.choice(n, k, replace=False) (base.py:406,413).  NumPy's implementation permutes all n
        indices per call (O(n)); for large panels draw k distinct indices by rejection instead (same law)."""
        if n <= 200000 or k * 20 > n:
            return np.random.choice(n, k, replace=False)
        while True:
            idx = np.random.randint(0, n, size=k)
            if len(np.unique(idx)) == k:
                return idx

    def egm_init(self, data, egm_n_iter=30000, batch_size=32, egm_batches_per_eval=500, verbose=1):
        """EGM warm start (base.py:380-431): g_d_freq WGAN-GP steps on the latent discriminator dz_net, then one
        step on g, e, f, h, per iteration.  Every step is one launch of the hand-written kernels of
        csrc/egm_kernels.h (forward, backward incl. the gradient-penalty double backward through the
        BatchNorm'd discriminator, Keras Adam).  The host draws the minibatch indices, the prior samples and the
        interpolation coefficients in the reference's order, one evaluation period at a time."""
        data_x, data_y, data_v = data
        n = len(data_x)
        eng = self.engine
        dev = eng.device
        p_ = self._p
        # Under torch.distributed the warm start is data parallel (north_star's collective, base.py:305-377): every rank holds ITS rows
        # of the panel, runs each step on its batch_size // world share of the global minibatch, and the discriminator / generator
        # gradients are all-reduced (RCCL) before the Adam step, so all ranks hold identical networks throughout.
        world, rank = parallel.world_size(), parallel.rank()
        lo_r, hi_r = parallel.shard_range(n)
        n_loc, b_loc = hi_r - lo_r, batch_size // world
        if world > 1 and b_loc < 2:
            raise ValueError("egm_init under torch.distributed: batch_size // world_size must be at least 2")
        # tests: ONE process steps on the minibatches a `_egm_emulate_world`-rank run forms (the ranks' shares side by side)
        emu = int(getattr(self, "_egm_emulate_world", 0)) if world == 1 else 0
        if emu > 1:
            b_loc = (batch_size // emu) * emu
        xd, yd, vd = self._dev(data_x[lo_r:hi_r]).reshape(-1), self._dev(data_y[lo_r:hi_r]).reshape(-1), self._dev(data_v[lo_r:hi_r])
        q = sum(p_["z_dims"])
        dims = [q] + list(p_["dz_units"]) + [1]
        dz = {"W": [_glorot(self._rs, dims[i], dims[i + 1]) for i in range(len(dims) - 1)],       # networks/base.py:338-363
              "b": [np.zeros(dims[i + 1], np.float32) for i in range(len(dims) - 1)],
              "gamma": [np.ones(dims[i + 1], np.float32) for i in range(len(dims) - 2)],
              "beta": [np.zeros(dims[i + 1], np.float32) for i in range(len(dims) - 2)]}
        self._push_weights()
        eng.egm_begin(b_loc, p_["dz_units"], p_["lr"], p_["use_z_rec"], dz)
        out_d = torch.zeros(2, device=dev)
        out_g = torch.zeros(6, device=dev)
        if world > 1:
            n_gen, n_dz = eng.egm_sizes()
            buf_g, buf_d = torch.empty(n_gen, device=dev), torch.empty(n_dz, device=dev)
        egm_log = []
        if verbose:
            print('EGM Initialization Starts ...')
        g_d_freq = int(p_['g_d_freq'])
        steps = g_d_freq + 1
        try:
            # Blocks of iterations up to and including the next evaluation point.  The host random numbers of block k + 1 are drawn
            # (reference order) on a worker thread, on a PRIVATE copy of the generator state, while the GPU runs block k and its
            # evaluation pass; np.random's global state moves only here, at hand-over, to where the sequential loop would have left
            # it (host_rng.EgmDrawPipeline: a block is redrawn if anything consumed np.random in between).
            blocks, bi = [], 0
            while bi <= egm_n_iter:
                stop = min(egm_n_iter, (bi // egm_batches_per_eval + 1) * egm_batches_per_eval if bi % egm_batches_per_eval else bi)
                blocks.append((bi, stop))
                bi = stop + 1

            pipe = host_rng.EgmDrawPipeline(n, batch_size, q, g_d_freq)
            pipe.request(blocks[0][1] - blocks[0][0] + 1)
            for kb, (batch_iter, stop) in enumerate(blocks):
                n_it = stop - batch_iter + 1
                idx_h, z_h, eps3 = pipe.take(blocks[kb + 1][1] - blocks[kb + 1][0] + 1 if kb + 1 < len(blocks) else 0)
                eps_h = eps3[:, :, 0]
                if world > 1:
                    idx_h, z_h = host_rng.egm_rank_share(idx_h, z_h, n, n_loc, b_loc, rank)
                elif emu > 1:
                    parts = []
                    for r in range(emu):
                        lo_e, hi_e = parallel.shard_range(n, r, emu)
                        parts.append(host_rng.egm_rank_share(idx_h, z_h, n, hi_e - lo_e, b_loc // emu, r)[0] + lo_e)
                    idx_h, z_h = np.ascontiguousarray(np.concatenate(parts, axis=2)), np.ascontiguousarray(z_h[:, :, :b_loc])
                idx_d, z_d = torch.from_numpy(idx_h).to(dev), torch.from_numpy(z_h).to(dev)
                for i in range(n_it if world == 1 else 0):
                    for j in range(g_d_freq):
                        eng.egm_disc_step(z_d[i, j], idx_d[i, j], vd, eps_h[i, j], out=out_d)
                    eng.egm_gen_step(z_d[i, g_d_freq], idx_d[i, g_d_freq], vd, xd, yd, out=out_g)
                for i in range(n_it if world > 1 else 0):
                    for j in range(g_d_freq):
                        eng.egm_disc_step(z_d[i, j], idx_d[i, j], vd, eps_h[i, j], apply=False, out=out_d)
                        eng.egm_grad(1, 1.0 / world, buf_d)
                        parallel.all_reduce_sum_(buf_d)                      # dz gradient of the global minibatch
                        eng.egm_apply(1, buf_d)
                    eng.egm_gen_step(z_d[i, g_d_freq], idx_d[i, g_d_freq], vd, xd, yd, apply=False, out=out_g)
                    eng.egm_grad(0, 1.0 / world, buf_g)
                    parallel.all_reduce_sum_(buf_g)                          # fused g | e | f | h gradient
                    eng.egm_apply(0, buf_g)
                batch_iter = stop
                if batch_iter % egm_batches_per_eval == 0:
                    eng.egm_sync()
                    self._pull_weights(("g", "f", "h", "e"))
                    if world > 1:                                            # the log line shows means over the global minibatch
                        parallel.all_reduce_sum_(out_g); parallel.all_reduce_sum_(out_d)
                        out_g /= world; out_d /= world
                    lg, ld = out_g.cpu().numpy(), out_d.cpu().numpy()
                    egm_log.append((batch_iter, float(lg[2])))          # l2_loss_z of this log line (diagnostics.py)
                    if verbose:
                        print('EGM Initialization Iter [%d] : e_loss_adv [%.4f], l2_loss_v [%.4f], l2_loss_z [%.4f], '
                              'l2_loss_x [%.4f], l2_loss_y [%.4f], g_e_loss [%.4f], dz_loss [%.4f], d_loss [%.4f]'
                              % (batch_iter, lg[0], lg[1], lg[2], lg[3], lg[4], lg[5], ld[0], ld[1]))
                    causal_pre, mse_x, mse_y, mse_v = self.evaluate(data=data)
                    if self._p['save_res'] and parallel.rank() == 0:
                        save_data('{}/causal_pre_egm_init_iter-{}.txt'.format(self.save_dir, batch_iter), causal_pre)
        finally:
            if 'pipe' in locals():
                pipe.close()
            eng.egm_end()
            self._pull_weights(("g", "f", "h", "e"))
        # (the thresholds describe the full-length warm start: a short one is merely unconverged and gets no diagnosis)
        self._egm_late_l2z = diagnostics.late_l2_loss_z([a for a, _ in egm_log], [b for _, b in egm_log], egm_n_iter) if (egm_log and egm_n_iter >= diagnostics.MIN_EGM_ITER) else None
        self._second_optimum_warned = False
        if verbose:
            print('EGM Initialization Ends.')

    def fit(self, data, epochs=100, epochs_per_eval=5, batch_size=32, startoff=0, use_egm_init=True,
            egm_n_iter=30000, egm_batches_per_eval=500, save_format='txt', verbose=1, z_adam=None, host_loop=False, dp_comm=None):
        """Iterative theta / Z updates (base.py:434-532).

        ``host_loop=False`` (single process): the minibatches of an epoch are issued by ONE library call (bgm_causal_fit_epoch), the
        latent phase of a minibatch overlapping the theta phase of the next on a second stream; ``True`` keeps the per-minibatch
        calls from Python (same results bit for bit).  Under torch.distributed over RCCL (one GPU per rank) the epoch is ONE library call
        too (bgm_causal_fit_epoch_dp: the gradient all-reduce is enqueued from C++ between the gradient tiles and the Adam step); other
        process groups (gloo) keep the host loop, where `parallel.all_reduce_sum_` sits between the calls.

        ``batch_size`` is the GLOBAL minibatch; under torch.distributed every rank owns a contiguous row
        shard, draws its share of each minibatch from its own rows, and the g/f/h gradients are
        all-reduced (RCCL) before the Adam step, so all ranks hold identical networks.
        ``z_adam`` -- the latent optimizer (base.py:246-302 applies a sparse gradient with Keras' Adam, whose sparse path decays the
        moments of and updates ALL rows at every minibatch):
          "replay" (default) the same recursion with the zero-gradient steps of the rows outside a minibatch deferred until the row
                   is next used (O(batch) per step; equal to "dense" up to fp32 rounding of a 256-term series, csrc/z_replay.h);
          "dense"  the recursion as Keras executes it: a sweep over the [N x q] table per minibatch (bit-faithful order of operations);
          "lazy"   batch rows only -- a different optimizer (build option)."""
        if z_adam is None:
            z_adam = "replay"
            diagnostics.notice_once("z_adam", "fit(z_adam=...) not given: the latent Adam runs in its replayed form ('replay': equal to Keras' "
                                    "dense-decay sweep up to fp32 rounding); 'dense' executes the sweep as the reference does (DESIGN_HISTORY.md section 4d)")
        if use_egm_init:
            self.egm_init(data, egm_n_iter=egm_n_iter, batch_size=batch_size,
                          egm_batches_per_eval=egm_batches_per_eval, verbose=verbose)
        data_x, data_y, data_v = data
        n_total = len(data_x)
        if self._p['save_res'] and parallel.rank() == 0:
            with open('{}/params.txt'.format(self.save_dir), 'w') as f_params:
                f_params.write(str(self.params))
        q = self.engine.q
        lo_r, hi_r = parallel.shard_range(n_total)
        if use_egm_init:
            if verbose:
                print('Initialize latent variables Z with e(V)...')
            data_z_init = None                                                          # base.py:479
        else:
            if verbose:
                print('Random initialization of latent variables Z...')
            data_z_init = np.random.normal(0, 1, size=(n_total, q)).astype('float32')   # base.py:482
        n_loc = hi_r - lo_r
        world = parallel.world_size()
        dev = self.engine.device
        x = self._dev(data_x[lo_r:hi_r]).reshape(-1)
        y = self._dev(data_y[lo_r:hi_r]).reshape(-1)
        v = self._dev(data_v[lo_r:hi_r])
        self.data_z = self.engine.encode(v) if data_z_init is None else self._dev(data_z_init[lo_r:hi_r])
        zm = torch.zeros_like(self.data_z)
        zv = torch.zeros_like(self.data_z)
        b_loc = max(1, batch_size // world)
        # Every rank must take the same number of steps with the same batch sizes (one all-reduce per step): an epoch uses the
        # first n_total // world entries of each rank's permutation; a rank that owns one row more leaves one (random) row out.
        n_use = n_total // world if world > 1 else n_loc
        eng = self.engine
        n_params = eng.fit_begin(n_loc, b_loc)
        if self._restored_opt is not None:
            if len(self._restored_opt["m"]) == n_params:
                eng.fit_state(self._restored_opt)      # g / f / h_optimizer slots and step counters of the restored checkpoint
            else:
                import warnings
                warnings.warn("bayesgm_amd: the restored checkpoint's optimizer slots (%d values) do not match this model's %d "
                              "parameters and are discarded: the fit starts with fresh Adam state" % (len(self._restored_opt["m"]), n_params))
        self._restored_opt = None
        self._fit_live = (zm, zv)
        grad = torch.empty(n_params, device=dev, dtype=torch.float32)
        loss = torch.zeros(8, device=dev, dtype=torch.float64)       # theta phase: row sums of loss_v, |v-mu|^2, loss_x, ...
        loss_z = torch.zeros(8, device=dev, dtype=torch.float64)     # Z phase: [6] = row sums of the negative log joint
        if z_adam not in ("dense", "lazy", "replay"):
            raise ValueError("z_adam must be 'replay', 'dense' or 'lazy'")
        lazy = {"dense": 0, "lazy": 1, "replay": 2}[z_adam]
        replay = (lazy == 2)
        lr_z = self._p['lr_z']
        best_loss = np.inf
        # one process per GPU over RCCL: the epoch stays ONE library call, with an RCCL communicator of the library's own
        # (parallel.DeviceComm) for the per-step gradient all-reduce; other process groups (gloo) keep the per-minibatch host loop
        # (``dp_comm``: a parallel.DeviceComm to use instead -- a one-rank communicator runs the data-parallel call in a single process)
        if dp_comm is None and world > 1 and host_loop is False:
            dp_comm = parallel.fit_comm(dev)
        self.last_fit_path = ("library_epoch_dp (RCCL all-reduce inside bgm_causal_fit_epoch_dp, %d ranks)" % dp_comm.world if dp_comm is not None
                              else "library_epoch" if (world == 1 and host_loop is False) else "host_loop")
        # per-epoch trace (row means over the epoch's minibatches; the reference shows the last minibatch in its progress bar)
        self.fit_history = []
        if verbose:
            print('Iterative Updating Starts ...')
        try:
            for epoch in range(epochs + 1):
                # permutation of the LOCAL rows (np.random.choice(N, N, replace=False), base.py:489)
                sample_idx = torch.from_numpy(np.random.choice(n_loc, n_loc, replace=False).astype(np.int32)).to(dev)
                loss.zero_()
                loss_z.zero_()
                n_rows = 0
                if dp_comm is not None:                        # data parallel: the loop AND the all-reduce inside the library
                    eng.fit_epoch_dp(dp_comm, x, y, v, self.data_z, zm, zv, sample_idx[:n_use], b_loc, self._p['lr_theta'], lr_z, lazy, loss, loss_z)
                    n_rows = n_use
                elif world == 1 and host_loop is False:        # the minibatch loop inside the library (bgm_causal_fit_epoch)
                    eng.fit_epoch(x, y, v, self.data_z, zm, zv, sample_idx[:n_use], b_loc, self._p['lr_theta'], lr_z, lazy, loss, loss_z)
                    n_rows = n_use
                for i in (range(0, n_use, b_loc) if n_rows == 0 else ()):
                    idx = sample_idx[i:min(i + b_loc, n_use)]
                    bg = int(idx.numel()) * world
                    if replay:
                        eng.fit_z_sync(self.data_z, zm, zv, idx, lr_z)           # this minibatch's rows, current before they are read
                    eng.fit_theta_grad(x, y, v, self.data_z, idx, bg, grad, loss)
                    parallel.all_reduce_sum_(grad)                       # C1: fused g|f|h gradient
                    eng.fit_theta_apply(grad, self._p['lr_theta'])
                    eng.fit_z_step(x, y, v, self.data_z, zm, zv, idx, bg, self._p['lr_z'], lazy, loss_z)
                    n_rows += int(idx.numel())
                l = loss.cpu().numpy() / max(1, n_rows)
                lz = loss_z.cpu().numpy() / max(1, n_rows)
                self.fit_history.append(dict(epoch=epoch, loss_v=float(l[0]), loss_mse_v=float(l[1] / eng.v_dim), loss_x=float(l[2]),
                                             loss_mse_x=float(l[3]), loss_y=float(l[4]), loss_mse_y=float(l[5]),
                                             loss_postrior_z=float(lz[6])))
                if verbose:
                    print('Epoch [%d/%d]: loss_px_z [%.4f], loss_mse_x [%.4f], loss_py_z [%.4f], loss_mse_y [%.4f], loss_pv_z [%.4f], '
                          'loss_mse_v [%.4f], loss_postrior_z [%.4f]' % (epoch, epochs, l[2], l[3], l[4], l[5], l[0], l[1] / eng.v_dim, lz[6]))
                if epoch % epochs_per_eval == 0:
                    if replay:
                        eng.fit_z_sync(self.data_z, zm, zv, None, lr_z)          # flush: evaluate / checkpoints read the whole table
                    causal_pre, mse_x, mse_y, mse_v = self._evaluate_dev(x, y, v, self.data_z, n_total, lo_r)
                    self.fit_history[-1].update(mse_x=float(mse_x), mse_y=float(mse_y), mse_v=float(mse_v))
                    if self.params.get('second_optimum_check', True):
                        self._second_optimum_warned = diagnostics.warn_if_second_optimum(getattr(self, '_egm_late_l2z', None), float(mse_v),
                                                                                         getattr(self, '_second_optimum_warned', False),
                                                                                         v_var=self._panel_v_var(v))
                    if verbose:
                        print('Epoch [%d/%d]: MSE_x: %.4f, MSE_y: %.4f, MSE_v: %.4f\n' % (epoch, epochs, mse_x, mse_y, mse_v))
                    if epoch >= startoff and mse_y < best_loss:
                        best_loss = mse_y
                        self.best_causal_pre = causal_pre
                        self.best_epoch = epoch
                        if self._p['save_model'] and parallel.rank() == 0:
                            self._pull_weights()
                            self.save_checkpoint(epoch)
                    if self._p['save_res'] and parallel.rank() == 0:
                        save_data('{}/causal_pre_at_{}.{}'.format(self.save_dir, epoch, save_format), causal_pre)
        finally:
            self._fit_live = None
            if replay:
                eng.fit_z_sync(self.data_z, zm, zv, None, lr_z)
            eng.fit_end()
            self._pull_weights()

    def save_checkpoint(self, epoch):
        """ckpt_manager.save(epoch) (base.py:527-529).  The archive holds what the reference's tf.train.Checkpoint tracks
        (:112-122) -- the parameters of g, e, f, h, and, when written from inside `fit`, the Adam slots and step counters of the
        g / f / h optimizers and the latent optimizer's step counter; at most 5 are kept."""
        flat = {}
        for k, net in self.nets.items():
            for i, (W, b) in enumerate(net):
                flat["%s_W%d" % (k, i)] = W
                flat["%s_b%d" % (k, i)] = b
        if self._fit_live is not None:
            st = self.engine.fit_state()
            # (the latent table and its slots are not among the objects the reference's tf.train.Checkpoint tracks, :112-122: a
            # restored model re-initialises Z with e(V) or N(0, I) in fit, as the reference does -- they are not written)
            flat.update(opt_m=st["m"], opt_v=st["v"], opt_steps=np.array([st["t_theta"], st["t_z"]], np.int64))
        flat["seed_state"] = np.array([self._base_seed, self._seed_counter], np.int64)
        flat.update(self._checkpoint_extra())
        path = self.ckpt_manager.save("ckpt-%s.npz" % epoch, flat)
        print('Saving checkpoint for epoch {} at {}'.format(epoch, path))
        return path

    def _checkpoint_extra(self):
        """Further tracked objects of a subclass (IdentifiableCausalBGM: prior_net, prior_optimizer) as named arrays."""
        return {}

    def _restore_extra(self, d):
        pass

    def load_checkpoint(self, path):
        d = np.load(path)
        self._restore_extra(d)
        for k in list(self.nets):
            self.nets[k] = [(d["%s_W%d" % (k, i)], d["%s_b%d" % (k, i)]) for i in range(len(self.nets[k]))]
        self._push_weights()
        if "opt_m" in d.files:
            self._restored_opt = dict(m=d["opt_m"], v=d["opt_v"], t_theta=int(d["opt_steps"][0]), t_z=int(d["opt_steps"][1]))
        if "seed_state" in d.files and int(d["seed_state"][0]) == self._base_seed:
            self._seed_counter = int(d["seed_state"][1])

    # ------------------------------------------------------------------ evaluate
    @staticmethod
    def _percentile_nearest(a, qpct):
        """tfp.stats.percentile default interpolation='nearest' (base.py:558-559)."""
        s = np.sort(np.asarray(a).ravel())
        return s[int(np.round((len(s) - 1) * qpct / 100.0))]

    def _evaluate_dev(self, x, y, v, z, n_total, lo_r, nb_intervals=200, x_full=None):
        """evaluate on this rank's rows + reduction over ranks.  Returns numpy (causal_pre, mse_x, mse_y, mse_v)."""
        eng = self.engine
        n_loc = v.shape[0]
        if self._p['binary_treatment']:
            sums, ite = eng.evaluate(x, y, v, z)
            parallel.all_reduce_sum_(sums)
            ite = parallel.all_gather_rows(ite.reshape(-1, 1), n_total)
            s = sums.cpu().numpy()
            return (ite.cpu().numpy(), np.float32(s[1] / n_total), np.float32(s[2] / n_total),
                    np.float32(s[0] / (n_total * self.engine.v_dim)))
        # dose grid between the 5th / 95th percentile of ALL x (base.py:558-560)
        xs_all = parallel.all_gather_rows(x.reshape(-1, 1), n_total).cpu().numpy() if x_full is None else x_full
        x_min = self._percentile_nearest(xs_all, 5.0)
        x_max = self._percentile_nearest(xs_all, 95.0)
        x_values = np.linspace(x_min, x_max, nb_intervals).astype(np.float32)
        sums, dose = eng.evaluate(x, y, v, z, x_values)
        dose = dose.double()
        parallel.all_reduce_sum_(sums)
        parallel.all_reduce_sum_(dose)
        s = sums.cpu().numpy()
        return ((dose / n_total).float().cpu().numpy(), np.float32(s[1] / n_total), np.float32(s[2] / n_total),
                np.float32(s[0] / (n_total * self.engine.v_dim)))

    def evaluate(self, data, data_z=None, nb_intervals=200):
        """(causal_pre, mse_x, mse_y, mse_v) (base.py:534-570); data_z=None -> e_net(data_v)."""
        data_x, data_y, data_v = data
        n_total = len(data_x)
        lo_r, hi_r = parallel.shard_range(n_total)
        x = self._dev(data_x[lo_r:hi_r]).reshape(-1)
        y = self._dev(data_y[lo_r:hi_r]).reshape(-1)
        v = self._dev(data_v[lo_r:hi_r])
        if data_z is None:
            z = self.engine.encode(v)
        else:
            z = self._dev(data_z[lo_r:hi_r]) if len(data_z) == n_total else self._dev(data_z)
        return self._evaluate_dev(x, y, v, z, n_total, lo_r, nb_intervals)

    # ------------------------------------------------------------------ predict
    def _sampling_options(self, reset, use_hmc, sampler_opts, own_checks, alpha, n_mcmc, x_values):
        """What predict, predict_individual, predict_new and predict_average do before they look at their data, in this order: the
        attributes named in ``reset`` are cleared; ``use_hmc()`` (None: always) says whether the HMC sampler runs, and its options
        ``sampler_opts = (step_size, n_leapfrog, mass, burn_in)`` are resolved and checked; ``own_checks(hmc in use)`` runs the
        method's own checks; then alpha, n_mcmc and the normalisation of ``x_values`` (None stays None).  Touches no device.
        -> (hmc, x_values, what own_checks returned), hmc = (step size, leapfrog steps, target acceptance rate, mass) or None."""
        for name in reset:
            setattr(self, name, None)
        step_size, n_leapfrog, mass, burn_in = sampler_opts
        hmc = None
        if use_hmc is None or use_hmc():
            hmc = hmc_mod.resolve(type(self).__name__, self._p, step_size, n_leapfrog, hmc_mod.DEFAULT_TARGET)
        mass = hmc_mod.check_mass(mass, hmc is not None, True, burn_in)
        own = own_checks(hmc is not None)
        if hmc is not None:
            hmc = hmc + (mass,)
        assert 0 < alpha < 1, "The significance level 'alpha' must be greater than 0 and less than 1."
        parallel.check_n_mcmc(n_mcmc)
        if x_values is not None:
            x_values = np.array([x_values], dtype=float) if np.isscalar(x_values) else np.array(x_values, dtype=float)
        return hmc, x_values, own

    def _begin_sampling(self, verbose):
        """The seed of a sampler call, drawn after every refusal that needs no device"""
        seed = self._next_seed()
        if verbose:
            print('MCMC Latent Variable Sampling ...')
        return seed

    def _sample_blocks(self, data, blocks, run, consume, verbose, sample=None, keep_mh_scale=False, **route_kw):
        """The loop over row blocks behind predict, predict_individual, predict_new and predict_average.  ``run = (burn_in, n_mcmc,
        seed, hmc)``, hmc as _sampling_options returns it.  Every block [s0, e0) of ``data = (x, y, v)`` goes to the device and is
        sampled by engine.hmc_sample with the route's keyword arguments ``route_kw`` -- by ``sample(x, y, v, s0)``, the caller's MH
        call, where hmc is None --; ``consume(s0, e0, x, out)`` takes what the block returned, and the block's steps, metric and
        acceptance tail are recorded.  Afterwards the acceptance rate is reported and the steps and the metric are gathered over
        the ranks into hmc_row_step_ / hmc_row_mass_ (the MH sampler's per-row scales into mh_row_scale_, with keep_mh_scale), and
        with a trajectory option among ``route_kw`` (_traj_kw) the rows' mean leapfrog steps into hmc_row_leapfrog_."""
        burn_in, n_mcmc, seed, hmc = run
        data_x, data_y, data_v = data
        eng, n_test, total_it = self.engine, len(data_x), burn_in + n_mcmc
        scale_key, scale_attr = ("row_step", "hmc_row_step_") if hmc is not None else ("row_scale", "mh_row_scale_" if keep_mh_scale else None)
        row_scale = torch.zeros(n_test, device=eng.device, dtype=torch.float32) if scale_attr else None
        row_mass = torch.zeros((n_test, eng.q), device=eng.device, dtype=torch.float32) if hmc is not None and hmc[3] is not None else None
        row_lf = torch.zeros(n_test, device=eng.device, dtype=torch.float32) if hmc is not None and "max_trajectory" in route_kw else None
        acc_tail = 0.0
        for (s0, e0) in blocks:
            x = self._dev(data_x[s0:e0]).reshape(-1)
            y = self._dev(data_y[s0:e0]).reshape(-1)
            v = self._dev(data_v[s0:e0])
            if hmc is not None:
                out = eng.hmc_sample(x, y, v, burn_in, n_mcmc, hmc[0], hmc[1], seed, row_base=s0, adapt=hmc[2], mass=hmc[3], **route_kw)
            else:
                out = sample(x, y, v, s0)
            consume(s0, e0, x, out)
            if row_scale is not None:
                row_scale[s0:e0] = out[scale_key]
            if row_mass is not None:
                row_mass[s0:e0] = out["mass_scale"]
            if row_lf is not None:
                row_lf[s0:e0] = out["row_leapfrog"]
            acc_tail += float(out["acc_count"][max(0, total_it - 100):].sum().item())
        self._report_acceptance(acc_tail, min(100, total_it), n_test, verbose)
        if row_scale is not None:
            setattr(self, scale_attr, parallel.all_reduce_sum_(row_scale).cpu().numpy())      # disjoint row sets: the sum is the gather
        if row_mass is not None:
            self.hmc_row_mass_ = parallel.all_reduce_sum_(row_mass).cpu().numpy()
        if row_lf is not None:
            self.hmc_row_leapfrog_ = parallel.all_reduce_sum_(row_lf).cpu().numpy()

    @staticmethod
    def _traj_kw(traj):
        """(max_trajectory as a float, jitter as 0 / 1) of causal_hmc.check_trajectory -> the keyword arguments of engine.hmc_sample;
        none when both are off, so that the run is the one without the options."""
        T, jit = traj
        return dict(max_trajectory=T if T > 0.0 else None, jitter=bool(jit)) if (T > 0.0 or jit) else {}

    def predict(self, data, alpha=0.01, n_mcmc=3000, burn_in=5000, x_values=None, q_sd=1.0, sample_y=True,
                bs=10000, verbose=1, diagnose_rows=0, row_adapt=False, sampler='mh', step_size=None, n_leapfrog=None,
                draw_budget_bytes=None, mass='identity', fused_effects=False, max_trajectory=None, jitter_leapfrog=False):
        """Causal effects with posterior intervals from latent MCMC samples (base.py:573-668).

        ``sampler='hmc'`` (opt-in; ``'mh'`` is the reference's sampler and the default): the latents are sampled by Hamiltonian Monte
        Carlo with ``n_leapfrog`` steps per transition and a step size per chain that starts from ``step_size`` and adapts during
        burn-in towards an acceptance rate of 0.75 (causal_hmc.py; None = that module's defaults).  This rank's rows are sampled in
        blocks whose retained draws fit ``draw_budget_bytes`` (default 2 GiB) and the effects are computed from each block's draws
        on the device; a chain depends on its own row only, so the block size does not change a row's draws.  ``q_sd`` is not
        used, ``row_adapt`` and a non-positive ``q_sd`` are refused, ``diagnose_rows`` works.  The steps are left in
        ``self.hmc_row_step_``.  ``mass='diag'`` (with ``sampler='hmc'``): every chain also estimates a scale per latent coordinate
        from its own burn-in draws (a diagonal metric, causal_hmc.py) and keeps it for the retained draws; the scales are left in
        ``self.hmc_row_mass_`` [n, q].  ``fused_effects=True`` (with ``sampler='hmc'``, opt-in): the effects are computed inside the
        sampling kernel after every retained decision and no draws are stored, so this rank's shard is sampled in one piece
        (``draw_budget_bytes`` has no meaning and is refused; a binary treatment keeps the cap on the ITE matrix).  Chains, steps,
        metric and seed sequence are those of the draws route, and so is the result whenever that route runs one block (several
        blocks reassociate the float32 sums over rows).  Generators too deep for the fused kernels' LDS raise the library's error.
        ``max_trajectory = T`` / ``jitter_leapfrog=True`` (with ``sampler='hmc'``, opt-in): a chain whose adapted step is eps takes
        only as many of the ``n_leapfrog`` steps as keep eps x steps below T (at least one), and with the jitter a number uniform on
        1 .. that many, drawn per chain and iteration (causal_hmc.resolve_trajectory); the cure for chains whose step grew until a
        trajectory returns to its start.  The mean steps per retained transition are left in ``self.hmc_row_leapfrog_`` [n].

        ``bs`` bounded the host memory of the reference; here all rows are sampled in one launch per
        segment (row-blocked only if the ITE draw matrix would exceed device memory) and the result does
        not depend on it.  Under torch.distributed the rows are sharded by rank and results gathered.

        ``diagnose_rows = k > 0`` (fixed ``q_sd`` only): after the run the chains of k rows are sampled once more with their
        draws kept, and their split R-hat / effective sample size stored in ``self.mcmc_diagnostics_``
        (diagnostics.ChainDiagnostics, row indices in ``.rows``); the result and the seed sequence are unchanged.

        ``row_adapt = True`` (target acceptance 0.25) or a target in (0, 1): every chain adapts a proposal scale of its own during
        burn-in (row_adapt.py), starting from ``q_sd`` (1.0 if ``q_sd`` is None or <= 0), and keeps it for the retained draws.  A
        chain depends on its own row only, so a rank's shard is sampled in one piece, the result does not depend on ``bs`` or the
        rank count, and ``diagnose_rows`` works.  The scales are left in ``self.mh_row_scale_``."""
        ra_target = self._row_adapt_target(row_adapt)
        hmc, x_values, traj = self._sampling_options(
            ("mh_row_scale_", "hmc_row_step_", "hmc_row_mass_", "hmc_row_leapfrog_"), lambda: hmc_mod.check_predict_options(sampler, q_sd, row_adapt),
            (step_size, n_leapfrog, mass, burn_in),
            lambda use_hmc: (hmc_mod.check_fused(fused_effects, use_hmc, draw_budget_bytes),
                             hmc_mod.check_trajectory(max_trajectory, jitter_leapfrog, use_hmc))[1],
            alpha, n_mcmc, x_values)
        binary = bool(self._p['binary_treatment'])
        if not binary and x_values is None:
            raise ValueError("For continuous treatment, 'x_values' must not be None. Provide a list or a single treatment value.")
        data_x, data_y, data_v = data
        n_test = len(data_x)
        bs = max(1, int(bs))
        adaptive = (q_sd is None) or (q_sd <= 0)
        if ra_target is not None:        # per-chain scales replace the block-wide one; q_sd is where they start
            q_sd, adaptive = row_adapt_mod.start_scale(q_sd), False
        diagnose_rows = int(diagnose_rows or 0)
        if diagnose_rows > 0 and adaptive:
            raise ValueError("predict(diagnose_rows=...) needs a fixed q_sd: with the adaptive scale (q_sd None or <= 0) every block's "
                             "scale schedule depends on the whole block's acceptance and cannot be reproduced from a window of rows")
        seed = self._begin_sampling(verbose)
        eng = self.engine
        dev = eng.device
        world, rank = parallel.world_size(), parallel.rank()
        # Row blocks.  A fixed proposal scale makes every chain independent of its block (the Philox stream is keyed by the
        # global row), so each rank samples its contiguous shard in one piece.  With the adaptive scale (q_sd <= 0) the
        # reference adapts q_sd per `bs`-block from that block's acceptance window (base.py:632-637, 880-893): the blocks are
        # the reference's [start, start + bs) and are dealt to the ranks whole.
        if adaptive:
            blocks = [(s0, min(s0 + bs, n_test)) for s0 in range(0, n_test, bs)][rank::world]
        else:
            lo_r, hi_r = parallel.shard_range(n_test)
            blocks = [(lo_r, hi_r)] if hi_r > lo_r else []
        if binary:        # keep the [rows x n_mcmc] draw matrix of one launch below ~32 GiB
            max_rows = max(16, int((32 << 30) // (4 * max(1, n_mcmc))))
            if not adaptive:
                blocks = [(s0, min(s0 + max_rows, e0)) for (b0, e0) in blocks for s0 in range(b0, e0, max_rows)]
        if hmc is not None:              # the retained draws of a block are kept: blocks within the draw budget (none kept when fused)
            blocks = hmc_mod.predict_blocks(blocks, n_mcmc, eng.q, draw_budget_bytes, fused_effects)
        if binary:
            res = torch.zeros((3, n_test), device=dev, dtype=torch.float32)     # mean, lower, upper (this rank's rows filled)
        else:
            sums = torch.zeros((len(x_values), n_mcmc), device=dev, dtype=torch.float64)   # adrf_draw_sums (base.py:660)
        # The effect of a block comes out of the sampler (the MH sampler, and HMC with fused_effects) or, on HMC's draws route, out
        # of engine.effects on the block's draws; either way it is accumulated below.
        effect_kw = dict(effect=_lib.EFFECT_ITE if binary else _lib.EFFECT_ADRF, x_values=x_values, sample_y=sample_y)
        from_draws = hmc is not None and not fused_effects

        def sample_mh(x, y, v, s0):
            return eng.mh_sample(x, y, v, burn_in, n_mcmc, q_sd, seed, row_base=s0, adaptive=adaptive, row_adapt=ra_target, **effect_kw)

        def consume(s0, e0, x, out):
            if from_draws:
                draws = out.pop("draws")
                if binary:
                    out["ite"] = eng.effects(x, draws, burn_in, seed, sample_y=sample_y, row_base=s0).t().contiguous()      # [rows, n_mcmc]
                else:
                    out["adrf"] = eng.effects(x, draws, burn_in, seed, x_values=x_values, sample_y=sample_y, row_base=s0)
            if binary:
                mean, lo, hi = eng.row_mean_quantiles(out["ite"], alpha / 2, 1 - alpha / 2)
                res[0, s0:e0], res[1, s0:e0], res[2, s0:e0] = mean, lo, hi
            else:
                sums.add_(out["adrf"].double() * float(e0 - s0))
        self._sample_blocks(data, blocks, (burn_in, n_mcmc, seed, hmc), consume, verbose, sample=sample_mh, keep_mh_scale=ra_target is not None,
                            **(dict(want_draws=True) if from_draws else effect_kw), **self._traj_kw(traj))
        if diagnose_rows > 0:
            self._diagnose_rows(data, diagnose_rows, burn_in, n_mcmc, q_sd, seed, row_adapt=ra_target, hmc=hmc, traj_kw=self._traj_kw(traj))
        if binary:
            parallel.all_reduce_sum_(res)                         # disjoint row sets: the sum is the gather
            res = res.cpu().numpy()
            return res[0], np.stack([res[1], res[2]], axis=1)
        parallel.all_reduce_sum_(sums)                            # C3: [n_doses x n_mcmc]
        causal_effects = (sums / float(n_test)).float().contiguous()
        adrf, lo, hi = eng.row_mean_quantiles(causal_effects, alpha / 2, 1 - alpha / 2)
        return adrf.cpu().numpy(), torch.stack([lo, hi], dim=1).cpu().numpy()

    def predict_individual(self, data, x_values, alpha=0.01, n_mcmc=3000, burn_in=5000, sample_y=True, step_size=None, n_leapfrog=None,
                           mass='identity', interval='normal', draw_budget_bytes=None, groups=None, verbose=1, max_trajectory=None,
                           jitter_leapfrog=False):
        """The dose-response curve of every row under a continuous treatment, with its posterior uncertainty: ``(mean [n, n_doses],
        interval [n, n_doses, 2])`` of y_i(x_k), the outcome of row i at dose ``x_values[k]``.  The reference has no counterpart
        (its continuous-treatment ``predict`` averages over the panel); a binary treatment has ``predict``'s ITE.

        The latents are always sampled by the HMC sampler of ``predict(sampler='hmc')`` (``step_size``, ``n_leapfrog``, ``mass`` and
        the seed sequence as there; the steps and the metric are left in ``self.hmc_row_step_`` / ``self.hmc_row_mass_``), and the
        outcome net runs inside the sampling kernel after every retained decision.  Per row and dose the kernel keeps the moments
        of the ``n_mcmc`` values; their standard deviations are left in ``self.individual_sd_`` [n, n_doses].

        ``interval='normal'`` (default): ``mean -/+ z(1 - alpha/2) * sd``.  This is a NORMAL APPROXIMATION of the posterior of
        y_i(x_k), not a quantile of its draws.  Nothing of size ``n_mcmc`` is stored and this rank's shard is sampled in one piece.
        ``interval='quantile'``: the exact ``alpha/2`` and ``1 - alpha/2`` quantiles of the stored draws; rows are sampled in blocks
        whose ``rows x n_doses x n_mcmc x 4`` bytes fit ``draw_budget_bytes`` (default 2 GiB).  ``mean`` and the sd still come from
        the moments, and a chain and its outcome noise depend on the row alone, so the blocks do not change a row's result.
        ``interval='tails'``: the bounds of ``'quantile'``, bit for bit, without the draws: per row and dose the sampling kernel keeps
        the ``K`` smallest and the ``K`` largest of the ``n_mcmc`` values (``K = causal_hmc.tail_size(alpha, n_mcmc)``, about
        ``alpha/2 * n_mcmc + 2``: 16 at the defaults), which is all the two interpolated quantiles read.  Rows are sampled in blocks
        whose ``rows x n_doses x K x 8`` bytes fit ``draw_budget_bytes``; ``mean``, the sd and ``groups`` as with ``'normal'``.

        ``groups`` (int labels [n], optional): ``self.group_dose_response_ = {label: (mean_g, sd_g)}``, the curve of every subgroup
        (causal_hmc.group_dose_response).  Under torch.distributed the rows are sharded by rank and the results gathered.

        ``max_trajectory`` / ``jitter_leapfrog``: as in ``predict(sampler='hmc')``, ``self.hmc_row_leapfrog_`` set as there; refused
        with ``interval='tails'``, whose kernels have no such variant."""
        hmc, x_values, traj = self._sampling_options(
            ("hmc_row_step_", "hmc_row_mass_", "hmc_row_leapfrog_", "individual_sd_", "group_dose_response_"), None,
            (step_size, n_leapfrog, mass, burn_in),
            lambda _: (hmc_mod.check_individual(bool(self._p['binary_treatment']), x_values, interval, draw_budget_bytes),
                       hmc_mod.check_trajectory(max_trajectory, jitter_leapfrog, True, interval))[1], alpha, n_mcmc,
            x_values)
        n_test = len(data[0])
        if groups is not None:
            hmc_mod.group_dose_response(np.zeros((n_test, 0)), np.zeros((n_test, 0)), groups)      # (the labels' checks, before a device is touched)
        mean, bounds = self._individual_rows(data, x_values, alpha, (burn_in, n_mcmc, hmc), sample_y, interval, draw_budget_bytes, verbose,
                                             traj=traj)
        if groups is not None:
            self.group_dose_response_ = hmc_mod.group_dose_response(mean, self.individual_sd_, groups)
        return mean, bounds

    def _individual_rows(self, data, x_values, alpha, run, sample_y, interval, draw_budget_bytes, verbose, partial=False, traj=(0.0, 0)):
        """The row blocks of predict_individual (and of predict_new for a continuous treatment, partial=True: NaN in data's x / y
        marks what a row does not observe): this rank's shard in the blocks of causal_hmc.individual_blocks, every block sampled with
        the per-row effects inside the kernel, the results gathered over the ranks -> (mean, bounds); run = (burn_in, n_mcmc, hmc);
        sets hmc_row_step_, hmc_row_mass_ and individual_sd_ (and, with the trajectory options traj, hmc_row_leapfrog_)."""
        (mean, sd), bounds, _ = self._row_series(data, x_values, alpha, run, sample_y, interval, draw_budget_bytes, verbose, partial, traj)
        self.individual_sd_ = sd
        return mean, bounds

    def _row_series(self, data, x_values, alpha, run, sample_y, interval, draw_budget_bytes, verbose, partial=False, traj=(0.0, 0),
                    kind=hmc_mod.RESULT_KINDS["rows"], **kind_kw):
        """What _individual_rows, predict_dose_effect and predict_best_dose share -> ((mean, sd) of y_i(x_k), bounds, None).  kind
        is the per-row record of causal_hmc.RESULT_KINDS whose kernels run (its `request` asks engine.hmc_sample for it; with
        interval='tails' the tails are those of that kind) and kind_kw the options of hmc_sample that are the kind's own.
        "contrasts": x_values[0] is the baseline, the kernels also keep c_i(k) = y_i(x_k) - y_i(x_0) per draw, the stored draws
        and the tails are those of c, and the result is ((mean, sd) of y, bounds of c, (mean, sd) of c).  "choice" (kind_kw:
        maximize, threshold | None): the kernels also compare the doses per draw, and the third item is (best_count [n, n_doses],
        best_ref [n], best_s1 [n], above_count [n, n_doses] | None), float64."""
        contrasts, choice = kind.name == "contrasts", kind.name == "choice"
        burn_in, n_mcmc, hmc = run
        n_test, n_doses = len(data[0]), len(x_values)
        seed = self._begin_sampling(verbose)
        eng = self.engine
        lo_r, hi_r = parallel.shard_range(n_test)
        quantile, tails = interval == 'quantile', interval == 'tails'
        k_tail = hmc_mod.tail_size(alpha, n_mcmc) if tails else None
        blocks = hmc_mod.individual_blocks([(lo_r, hi_r)] if hi_r > lo_r else [], n_mcmc, n_doses, interval, draw_budget_bytes, k_tail)
        nb = 4 if quantile or tails else 2
        # mean, sd(, lower, upper)(, contrast mean, contrast sd): this rank's rows filled
        res = torch.zeros((nb + (2 if contrasts else 0), n_test, n_doses), device=eng.device, dtype=torch.float64)
        draws_key = "contrast_draws" if contrasts else "row_draws"
        if choice:      # best_count, above_count [n, n_doses]; best_ref, best_s1 [n]: this rank's rows filled
            cnt = torch.zeros((2, n_test, n_doses), device=eng.device, dtype=torch.float64)
            bst = torch.zeros((2, n_test), device=eng.device, dtype=torch.float64)

        def consume(s0, e0, x, out):
            res[0, s0:e0], res[1, s0:e0] = out["row_mean"], out["row_sd"]
            if choice:
                cnt[0, s0:e0], bst[0, s0:e0], bst[1, s0:e0] = out["best_count"].double(), out["best_ref"].double(), out["best_s1"].double()
                if kind_kw["threshold"] is not None:
                    cnt[1, s0:e0] = out["above_count"].double()
            if contrasts:
                res[nb, s0:e0], res[nb + 1, s0:e0] = out["contrast_mean"], out["contrast_sd"]
            if quantile:
                _, lo, hi = eng.row_mean_quantiles(out.pop(draws_key).reshape((e0 - s0) * n_doses, n_mcmc), alpha / 2, 1 - alpha / 2)
                res[2, s0:e0], res[3, s0:e0] = lo.reshape(e0 - s0, n_doses).double(), hi.reshape(e0 - s0, n_doses).double()
            if tails:      # [2, K, n_doses, rows] -> bounds [n_doses, rows]
                lo, hi = eng.row_tail_quantiles(out.pop("tails"), n_mcmc, alpha / 2, 1 - alpha / 2)
                res[2, s0:e0], res[3, s0:e0] = lo.t().double(), hi.t().double()
        self._sample_blocks(data, blocks, (burn_in, n_mcmc, seed, hmc), consume, verbose, row_draws=quantile, row_tails=k_tail,
                            x_values=x_values, sample_y=sample_y, partial=partial, **kind.request, **kind_kw, **self._traj_kw(traj))
        res = parallel.all_reduce_sum_(res).cpu().numpy()
        mean, sd = res[0], res[1]
        contrast = (res[nb], res[nb + 1]) if contrasts else None
        if choice:
            cnt, bst = parallel.all_reduce_sum_(cnt).cpu().numpy(), parallel.all_reduce_sum_(bst).cpu().numpy()
            contrast = (cnt[0], bst[0], bst[1], cnt[1] if kind_kw["threshold"] is not None else None)
        if quantile or tails:
            bounds = np.stack([res[2], res[3]], axis=-1)
        else:
            z = NormalDist().inv_cdf(1.0 - alpha / 2)
            c_mean, c_sd = contrast if contrasts else (mean, sd)
            bounds = np.stack([c_mean - z * c_sd, c_mean + z * c_sd], axis=-1)
        return (mean, sd), bounds, contrast

    dose_effect_sd_ = None           # predict_dose_effect: posterior sd [n, n_doses] of the contrasts
    dose_effect_curve_ = None        # predict_dose_effect: (mean, sd), each [n, 1 + n_doses], of y_i at [baseline] + x_values
    group_dose_effect_ = None        # predict_dose_effect(groups=...): {label: (mean [n_doses], sd [n_doses])}; None otherwise

    def predict_dose_effect(self, data, x_values, baseline, alpha=0.01, n_mcmc=3000, burn_in=5000, sample_y=True, step_size=None,
                            n_leapfrog=None, mass='identity', interval='normal', draw_budget_bytes=None, groups=None, partial=False,
                            verbose=1):
        """The effect of a dose against a baseline dose for every row under a continuous treatment, with its posterior uncertainty:
        ``(effect [n, n_doses], interval [n, n_doses, 2])`` of y_i(x_values[k]) - y_i(baseline), what row i gains at dose
        ``x_values[k]`` over ``baseline`` (a finite scalar).  The reference has no counterpart; a binary treatment has ``predict``'s
        ITE.  ``predict_individual`` cannot give this: its moments and tails describe every dose alone, while the two doses of a
        contrast are evaluated on the same latent draw and are strongly correlated.  Here the sampling kernel forms the difference
        on every retained draw and keeps its moments (and, where asked, its draws or its tails), so nothing of size ``n_mcmc`` is
        stored with ``interval='normal'`` or ``'tails'``.

        The latents are sampled as in ``predict_individual`` (``step_size``, ``n_leapfrog``, ``mass`` and the seed sequence as there;
        ``self.hmc_row_step_`` / ``self.hmc_row_mass_`` set as there) at the doses ``[baseline] + x_values``; the baseline's own
        column, exactly zero, is dropped from what is returned.  ``self.dose_effect_sd_`` [n, n_doses] is the sd of the contrasts and
        ``self.dose_effect_curve_ = (mean, sd)``, each [n, 1 + n_doses], the curve of y_i at ``[baseline] + x_values``: what
        ``predict_individual`` returns there, bit for bit.

        ``interval``: ``'normal'`` | ``'quantile'`` | ``'tails'`` with ``predict_individual``'s meanings and row blocks
        (``draw_budget_bytes``), applied to the series of the contrast; ``'tails'`` gives the bounds of ``'quantile'`` bit for bit.
        With ``sample_y=True`` the interval is that of the DIFFERENCE OF TWO INDEPENDENT PREDICTIVE DRAWS: the outcomes at the two
        doses share the latent draw and carry their own outcome noise, as the two arms of the binary ITE do; ``sample_y=False``
        gives the interval of the difference of the two conditional means.

        ``groups`` (int labels [n], optional): ``self.group_dose_effect_ = {label: (mean_g, sd_g)}`` of the contrast
        (causal_hmc.group_dose_response).  ``partial=True``: NaN in ``data``'s y, or x and y, marks what a row does not observe, as
        in ``hmc_sampler(..., partial=True)`` -- new units: what would this patient gain from dose b over dose a; a row with its
        outcome observed and its treatment not, and NaN among the covariates, are refused.  The trajectory options are not taken:
        the contrast kernels have no such variant."""
        hmc, x_values, baseline = self._sampling_options(
            ("hmc_row_step_", "hmc_row_mass_", "hmc_row_leapfrog_", "dose_effect_sd_", "dose_effect_curve_", "group_dose_effect_"), None,
            (step_size, n_leapfrog, mass, burn_in),
            lambda _: hmc_mod.check_dose_effect(bool(self._p['binary_treatment']), x_values, baseline, interval, draw_budget_bytes),
            alpha, n_mcmc, x_values)
        n_test = len(data[0])
        if groups is not None:
            hmc_mod.group_dose_response(np.zeros((n_test, 0)), np.zeros((n_test, 0)), groups)      # (the labels' checks, before a device is touched)
        if partial:
            data = hmc_mod.check_partial_panel(*data)
        doses = np.concatenate([[baseline], x_values.reshape(-1)])
        curve, bounds, (c_mean, c_sd) = self._row_series(data, doses, alpha, (burn_in, n_mcmc, hmc), sample_y, interval, draw_budget_bytes,
                                                         verbose, partial=bool(partial), kind=hmc_mod.RESULT_KINDS["contrasts"])
        self.dose_effect_curve_ = curve
        effect, self.dose_effect_sd_, bounds = c_mean[:, 1:], c_sd[:, 1:], bounds[:, 1:]
        if groups is not None:
            self.group_dose_effect_ = hmc_mod.group_dose_response(effect, self.dose_effect_sd_, groups)
        return effect, bounds

    dose_regret_ = None              # predict_best_dose: expected regret [n, n_doses] of giving dose k
    dose_exceed_prob_ = None         # predict_best_dose(threshold=...): P(y_i(x_k) > threshold) [n, n_doses]; None otherwise
    dose_choice_curve_ = None        # predict_best_dose: (mean, sd), each [n, n_doses], of y_i at x_values
    group_dose_choice_ = None        # predict_best_dose(groups=...): {label: (share [n_doses], mean prob_best [n_doses])}; None otherwise

    def predict_best_dose(self, data, x_values, maximize=True, threshold=None, n_mcmc=3000, burn_in=5000, sample_y=False, step_size=None,
                          n_leapfrog=None, mass='identity', groups=None, partial=False, verbose=1):
        """Which dose is best for every row under a continuous treatment, and how sure the posterior is of it: ``(choice [n],
        prob_best [n, n_doses])``.  ``prob_best[i, k]`` is the share of the ``n_mcmc`` retained draws at which dose ``x_values[k]``
        gave row i its best outcome -- the largest with ``maximize=True``, the smallest otherwise, the lowest dose index on ties --;
        rows sum to 1.  ``choice[i]`` is the dose index with the best posterior mean (lowest index on ties): the Bayes choice under
        a linear utility, and the argmin of the expected regret up to float32 rounding.  The reference has no counterpart; a binary
        treatment has ``predict``'s ITE.  None of this follows from ``predict_individual``'s moments or tails or from
        ``predict_dose_effect``'s contrasts against one baseline: the best dose changes from draw to draw, so the sampling kernel
        compares the doses on every retained draw and keeps counts.  Nothing of size ``n_mcmc`` is stored and this rank's shard is
        sampled in one piece.

        ``self.dose_regret_`` [n, n_doses]: what is lost in expectation by giving dose k, ``E[best] - mean_k`` (``mean_k - E[best]``
        when minimising), with ``E[best]`` the posterior mean of the per-draw best outcome.  It is not clipped: it may be negative by
        float32 rounding only.  ``threshold`` (a finite scalar, optional): ``self.dose_exceed_prob_`` [n, n_doses] is the posterior
        probability that the outcome at dose k exceeds it.  ``self.dose_choice_curve_ = (mean, sd)``: what ``predict_individual``
        returns at ``x_values``, bit for bit.

        ``sample_y=False`` IS THE DEFAULT HERE: a decision compares the conditional means of the doses.  With ``sample_y=True``
        every dose carries its own INDEPENDENT predictive noise on the shared latent draw, as in ``predict_dose_effect``:
        ``prob_best`` is then the probability that one future outcome at dose k beats independent future outcomes at the others.

        The latents are sampled as in ``predict_individual`` (``step_size``, ``n_leapfrog``, ``mass`` and the seed sequence as
        there; ``self.hmc_row_step_`` / ``self.hmc_row_mass_`` set as there).  ``groups`` (int labels [n], optional):
        ``self.group_dose_choice_ = {label: (share of the group's rows choosing each dose, mean prob_best)}``
        (causal_hmc.group_dose_choice).  ``partial=True``: NaN in ``data``'s y, or x and y, marks what a row does not observe, as
        in ``predict_dose_effect`` -- new units; ``partial=True`` with ``mass='diag'`` on a model of more than 11 latent features is
        refused (``ValueError``): that one kernel is not built.  The trajectory options are not taken: the choice kernels have no such
        variant."""
        hmc, x_values, threshold = self._sampling_options(
            ("hmc_row_step_", "hmc_row_mass_", "hmc_row_leapfrog_", "dose_regret_", "dose_exceed_prob_", "dose_choice_curve_",
             "group_dose_choice_"), None, (step_size, n_leapfrog, mass, burn_in),
            lambda _: hmc_mod.check_best_dose(bool(self._p['binary_treatment']), x_values, threshold), 0.5, n_mcmc, x_values)
        n_test = len(data[0])
        if groups is not None:
            hmc_mod.group_dose_choice(np.zeros(n_test, np.int64), np.zeros((n_test, 0)), groups)      # (the labels' checks, before a device is touched)
        if partial and hmc[3] is not None:      # (the one combination whose kernel is not built)
            hmc_mod.check_choice_kernel(sum(self._p['z_dims']), True, True)
        if partial:
            data = hmc_mod.check_partial_panel(*data)
        maximize = bool(maximize)
        (mean, sd), _, (count, ref, s1, above) = self._row_series(data, x_values.reshape(-1), 0.5, (burn_in, n_mcmc, hmc), sample_y, 'normal',
                                                                  None, verbose, partial=bool(partial), kind=hmc_mod.RESULT_KINDS["choice"],
                                                                  maximize=maximize, threshold=threshold)
        self.dose_choice_curve_ = (mean, sd)
        prob_best, _, self.dose_regret_ = hmc_mod.choice_finalize(count, ref, s1, mean, n_mcmc, maximize)
        if above is not None:
            self.dose_exceed_prob_ = above / float(n_mcmc)
        choice = np.argmax(mean if maximize else -mean, axis=1)
        if groups is not None:
            self.group_dose_choice_ = hmc_mod.group_dose_choice(choice, prob_best, groups)
        return choice, prob_best

    def predict_new(self, data_v, data_x=None, x_values=None, alpha=0.01, n_mcmc=3000, burn_in=5000, sample_y=True, step_size=None,
                    n_leapfrog=None, mass='identity', interval='normal', draw_budget_bytes=None, verbose=1, max_trajectory=None,
                    jitter_leapfrog=False):
        """Effects for NEW units, whose outcome is not observed: the covariates ``data_v`` [n, p], perhaps the treatment ``data_x``
        [n] (None: not known for any row; NaN entries: not known for those rows), never the outcome.  The reference has no
        counterpart (its ``predict`` takes the triplet (x, y, v) of every row).

        The latent posterior of such a row is p(z | x, v), or p(z | v) without the treatment: the log posterior of ``predict``
        with the outcome term, and the treatment term where x is not known, left out.  It is sampled by the HMC sampler of
        ``predict(sampler='hmc')`` (``step_size``, ``n_leapfrog``, ``mass`` and the seed sequence as there; the steps and the metric
        are left in ``self.hmc_row_step_`` / ``self.hmc_row_mass_``) and the outcome net runs inside the sampling kernel.

        Continuous treatment (``x_values`` required): what ``predict_individual`` returns, ``(mean [n, n_doses], interval
        [n, n_doses, 2])`` of y_i(x_k), the sd in ``self.individual_sd_``; ``interval`` (``'tails'`` included) and
        ``draw_budget_bytes`` as there.
        Binary treatment: what ``predict`` returns, ``(ite [n], interval [n, 2])``, from the fused ITE kernel; ``interval=
        'quantile'`` gives ``predict``'s quantiles of the ITE draws, ``'normal'`` (default) ``mean -/+ z(1 - alpha/2) * sd`` of
        them (sd in ``self.individual_sd_`` [n]); the [rows x n_mcmc] ITE matrix of a block fits ``draw_budget_bytes`` (default
        2 GiB); ``'tails'`` is refused (the ITE route keeps no tails).  A row's result depends on (seed, its global row, its data) only; under torch.distributed the rows are sharded by
        rank and the results gathered.

        ``max_trajectory`` / ``jitter_leapfrog``: as in ``predict(sampler='hmc')``, ``self.hmc_row_leapfrog_`` set as there; refused
        with ``interval='tails'``.  The posterior of a new unit is close to the prior, so its chain's step grows furthest: these
        are the rows the cap is for."""
        binary = bool(self._p['binary_treatment'])
        hmc, x_values, ((data_v, data_x, data_y), traj) = self._sampling_options(
            ("hmc_row_step_", "hmc_row_mass_", "hmc_row_leapfrog_", "individual_sd_"), None, (step_size, n_leapfrog, mass, burn_in),
            lambda _: (hmc_mod.check_new(binary, data_v, data_x, x_values, interval, draw_budget_bytes),
                       hmc_mod.check_trajectory(max_trajectory, jitter_leapfrog, True, interval)), alpha, n_mcmc,
            None if binary else x_values)
        data = (data_x, data_y, data_v)
        if not binary:
            return self._individual_rows(data, x_values, alpha, (burn_in, n_mcmc, hmc), sample_y, interval, draw_budget_bytes, verbose,
                                         partial=True, traj=traj)
        n_test = len(data_x)
        seed = self._begin_sampling(verbose)
        eng = self.engine
        lo_r, hi_r = parallel.shard_range(n_test)
        rows = hmc_mod.block_rows(n_mcmc, 1, draw_budget_bytes)      # the ITE matrix [rows x n_mcmc] of one block
        blocks = [(s0, min(s0 + rows, hi_r)) for s0 in range(lo_r, hi_r, rows)]
        res = torch.zeros((4, n_test), device=eng.device, dtype=torch.float64)      # mean, sd, lower, upper (this rank's rows filled)

        def consume(s0, e0, x, out):
            ite = out.pop("ite")
            mean, lo, hi = eng.row_mean_quantiles(ite, alpha / 2, 1 - alpha / 2)
            res[0, s0:e0], res[2, s0:e0], res[3, s0:e0] = mean.double(), lo.double(), hi.double()
            res[1, s0:e0] = ite.double().std(dim=1) if n_mcmc > 1 else 0.0
        self._sample_blocks(data, blocks, (burn_in, n_mcmc, seed, hmc), consume, verbose, effect=_lib.EFFECT_ITE, sample_y=sample_y,
                            partial=True, **self._traj_kw(traj))
        res = parallel.all_reduce_sum_(res).cpu().numpy()
        mean, sd = res[0], res[1]
        self.individual_sd_ = sd
        if interval == 'quantile':
            return mean, np.stack([res[2], res[3]], axis=1)
        z = NormalDist().inv_cdf(1.0 - alpha / 2)
        return mean, np.stack([mean - z * sd, mean + z * sd], axis=1)

    average_effects_ = None          # predict_average: dict(ate, att, atc, *_interval, *_draws, counts, groups)

    def predict_average(self, data, alpha=0.01, n_mcmc=3000, burn_in=5000, sample_y=True, groups=None, estimand='ate', sampler='hmc',
                        q_sd=1.0, step_size=None, n_leapfrog=None, mass='identity', verbose=1):
        """Average effects of a binary treatment with posterior intervals: ``(effect, interval)`` of ``estimand`` = ``'ate'`` (all
        rows), ``'att'`` (the treated rows, x_i = 1) or ``'atc'`` (the control rows), the average of the individual treatment
        effect over those rows.  The reference has no counterpart (its tutorial takes ``mean(ITE)`` of ``predict``: a point estimate);
        a continuous treatment has ``predict``'s ADRF.

        For every retained draw the ITE is averaged over the rows FIRST; the effect is the mean of the ``n_mcmc`` per-draw averages
        and the interval their ``alpha / 2`` and ``1 - alpha / 2`` quantiles (linear interpolation, as ``predict``'s ADRF).  Without
        ``groups`` the result is ``(float, [2])``; with ``groups`` (int labels [n], at most 32 distinct) it is ``([n_groups],
        [n_groups, 2])`` in the order of the sorted distinct labels: the subgroup effects (CATE).  All three estimands, their
        per-draw series [n_groups, n_mcmc], the row counts [n_groups, 2] (control, treated) and the group labels are left in
        ``self.average_effects_``; an estimand without rows in a group is nan there and raises when it is the one asked for.

        ``sampler='hmc'`` (default): the HMC sampler of ``predict(sampler='hmc', fused_effects=True)`` -- ``step_size``,
        ``n_leapfrog``, ``mass`` and the seed sequence as there, ``self.hmc_row_step_`` / ``self.hmc_row_mass_`` set as there -- with
        the ITE summed by (group, arm) inside the sampling kernel: neither draws nor an ITE matrix are stored and this rank's shard
        is sampled in one piece.  ``sampler='mh'``: the MH sampler call of ``predict`` with a fixed ``q_sd`` and its cap on the ITE
        matrix; the matrix of every block is reduced by label on the device.  Under torch.distributed the rows are sharded by rank
        and the per-draw sums (float64) and counts are all-reduced."""
        def use_hmc():
            if hmc_mod.check_predict_options(sampler, q_sd, False):
                return True
            if q_sd is None or not float(q_sd) > 0:
                raise ValueError("predict_average needs a fixed q_sd > 0 with sampler='mh': the block-wide adaptive scale depends on "
                                 "predict's bs blocks; got %r" % (q_sd,))
            return False
        hmc, _, (group_labels, group_index) = self._sampling_options(
            ("average_effects_", "hmc_row_step_", "hmc_row_mass_"), use_hmc, (step_size, n_leapfrog, mass, burn_in),
            lambda _: hmc_mod.check_average(bool(self._p['binary_treatment']), estimand, groups, len(data[0])), alpha, n_mcmc, None)
        data_x, data_y, data_v = data
        n_test = len(data_x)
        n_groups = 1 if group_labels is None else len(group_labels)
        n_labels = 2 * n_groups
        labels = hmc_mod.average_labels(group_index, data_x)
        seed = self._begin_sampling(verbose)
        eng = self.engine
        dev = eng.device
        lo_r, hi_r = parallel.shard_range(n_test)
        blocks = [(lo_r, hi_r)] if hi_r > lo_r else []
        if hmc is None:                  # the [rows x n_mcmc] ITE matrix of one launch stays below ~32 GiB, as in predict
            max_rows = max(16, int((32 << 30) // (4 * max(1, n_mcmc))))
            blocks = [(s0, min(s0 + max_rows, e0)) for (b0, e0) in blocks for s0 in range(b0, e0, max_rows)]
        sums = torch.zeros((n_labels, n_mcmc), device=dev, dtype=torch.float64)
        counts = torch.from_numpy(hmc_mod.average_counts(labels[lo_r:hi_r], n_groups)).to(dev)

        def sample_mh(x, y, v, s0):
            return eng.mh_sample(x, y, v, burn_in, n_mcmc, q_sd, seed, effect=_lib.EFFECT_ITE, sample_y=sample_y, row_base=s0, adaptive=False,
                                 row_adapt=None)

        def consume(s0, e0, x, out):
            sums.add_(out["group_sums"].double() if hmc is not None else eng.ite_group_sums(out.pop("ite"), labels[s0:e0], n_labels))
        # (HMC samples this rank's shard in one block, so its labels are that block's)
        self._sample_blocks(data, blocks, (burn_in, n_mcmc, seed, hmc), consume, verbose, sample=sample_mh, effect=_lib.EFFECT_GROUP_ITE,
                            labels=labels[lo_r:hi_r], n_labels=n_labels, sample_y=sample_y)
        sums = parallel.all_reduce_sum_(sums).cpu().numpy().reshape(n_groups, 2, n_mcmc)
        counts = parallel.all_reduce_sum_(counts).cpu().numpy()
        series = hmc_mod.combine_average_effects(sums, counts)
        res = dict(counts=counts.astype(np.int64), groups=None if group_labels is None else np.array(group_labels))
        for name in hmc_mod.ESTIMANDS:
            res[name], res[name + "_interval"] = hmc_mod.average_summary(series[name], alpha)
            res[name + "_draws"] = series[name]
        self.average_effects_ = res
        hmc_mod.check_average_estimand(estimand, res[estimand], group_labels)
        if group_labels is None:
            return float(res[estimand][0]), res[estimand + "_interval"][0]
        return res[estimand], res[estimand + "_interval"]

    @staticmethod
    def _diagnose_windows(n_test, k):
        """Up to 8 evenly spaced contiguous row windows [start, stop) over the panel holding k rows in all (all rows when
        k >= n_test)."""
        k = min(int(k), n_test)
        if k <= 0:
            return []
        n_win = min(8, k)
        sizes = [k // n_win + (1 if i < k % n_win else 0) for i in range(n_win)]
        if n_win == 1:
            return [(0, sizes[0])]
        # window i starts at the i-th of n_win evenly spaced positions of [0, n_test - size_last]; the starts are at least one
        # window apart because n_test >= k
        wins, prev_stop = [], 0
        for i, sz in enumerate(sizes):
            start = max(prev_stop, (i * (n_test - sizes[-1])) // (n_win - 1))
            start = min(start, n_test - sum(sizes[i:]))
            wins.append((start, start + sz))
            prev_stop = start + sz
        return wins

    def _row_adapt_target(self, row_adapt):
        """row_adapt of predict / adaptive_sd='row' -> None or the target acceptance rate; ValueError where the per-chain scale does
        not exist (needs no device)."""
        target = row_adapt_mod.resolve_target(row_adapt)
        if target is not None:
            row_adapt_mod.check_supported(type(self).__name__, self._p)
        return target

    def _refuse_hmc(self, sampler, q_sd, row_adapt, step_size, n_leapfrog, mass='identity', fused_effects=False):
        """predict of the subclasses without an HMC path: sampler='hmc' raises the ValueError that names what is in the way (and so
        do a mass and a fused_effects that belong to it)."""
        if hmc_mod.check_predict_options(sampler, q_sd, row_adapt):
            hmc_mod.resolve(type(self).__name__, self._p, step_size, n_leapfrog, hmc_mod.DEFAULT_TARGET)
            raise ValueError("sampler='hmc' is not available for %s" % type(self).__name__)
        hmc_mod.check_mass(mass, False)
        hmc_mod.check_fused(fused_effects, False, None)

    def _adaptive_sd_target(self, adaptive_sd, target_acceptance_rate):
        """adaptive_sd of metropolis_hastings_sampler -> None (None / bool: the fixed or the block-wide scale) or, for 'row', the
        target acceptance rate of the per-chain scale; ValueError for another string or where that scale does not exist."""
        if not isinstance(adaptive_sd, str):
            return None
        if adaptive_sd != 'row':
            raise ValueError("adaptive_sd must be None, a bool or 'row'; got %r" % (adaptive_sd,))
        row_adapt_mod.check_supported(type(self).__name__, self._p)
        return self._row_adapt_target(target_acceptance_rate)

    def _diagnose_rows(self, data, k, burn_in, n_mcmc, q_sd, seed, row_adapt=None, hmc=None, traj_kw=None):
        """Re-run the chains of k rows of predict's panel with their draws kept (the Philox stream is keyed by the global row, so
        with the same seed and row_base these are the chains predict ran) and store their diagnostics.  Every rank computes the
        same windows; no collectives and no new seed."""
        data_x, data_y, data_v = data
        eng = self.engine
        parts, rows = [], []
        for (s0, e0) in self._diagnose_windows(len(data_x), k):
            xyv = (self._dev(data_x[s0:e0]).reshape(-1), self._dev(data_y[s0:e0]).reshape(-1), self._dev(data_v[s0:e0]))
            if hmc is not None:
                out = eng.hmc_sample(*xyv, burn_in, n_mcmc, hmc[0], hmc[1], seed, want_draws=True, row_base=s0, adapt=hmc[2], mass=hmc[3],
                                     **(traj_kw or {}))
            else:
                out = eng.mh_sample(*xyv, burn_in, n_mcmc, q_sd, seed, want_draws=True, row_base=s0, row_adapt=row_adapt)
            parts.append(out["draws"])
            rows.append(np.arange(s0, e0))
        d = diagnostics.chain_diagnostics(torch.cat(parts, dim=1))
        d.rows = np.concatenate(rows)
        self.mcmc_diagnostics_ = d
        diagnostics.warn_if_not_mixed(d, self.params, "CausalBGM.predict")

    def _report_acceptance(self, acc_tail, window, n_test, verbose):
        t = torch.tensor([acc_tail], dtype=torch.float64, device=self.engine.device)
        parallel.all_reduce_sum_(t)
        self.last_acceptance_rate = float(t.item()) / (window * n_test)
        if verbose:
            print(f"Final MCMC Acceptance Rate: {self.last_acceptance_rate:.4f}")

    def metropolis_hastings_sampler(self, data, initial_q_sd=1.0, q_sd=None, burn_in=5000, n_keep=3000,
                                    target_acceptance_rate=0.25, tolerance=0.05, adjustment_interval=50,
                                    adaptive_sd=None, window_size=100, diagnostics=False):
        """Posterior samples of Z, shape (n_keep, n, q) (base.py:820-904).  diagnostics=True: split R-hat / effective sample
        size of every chain, computed on the device before the copy to the host, in ``self.mcmc_diagnostics_``.

        ``adaptive_sd='row'``: every chain adapts a proposal scale of its own during burn-in towards ``target_acceptance_rate``
        (row_adapt.py), starting from ``q_sd`` if positive, else ``initial_q_sd``; the scales are left in ``self.mh_row_scale_``."""
        data_x, data_y, data_v = data
        ra_target = self._adaptive_sd_target(adaptive_sd, target_acceptance_rate)
        self.mh_row_scale_ = None
        if ra_target is not None:
            q_sd, adaptive_sd = row_adapt_mod.start_scale(q_sd, initial_q_sd), False
        if adaptive_sd is None:
            adaptive_sd = (q_sd is None or q_sd <= 0)
        out = self.engine.mh_sample(self._dev(data_x).reshape(-1), self._dev(data_y).reshape(-1), self._dev(data_v),
                                    burn_in, n_keep, q_sd, self._next_seed(), want_draws=True, adaptive=adaptive_sd,
                                    initial_q_sd=initial_q_sd, target=target_acceptance_rate, tol=tolerance,
                                    adj_int=adjustment_interval, window=window_size, row_adapt=ra_target)
        if ra_target is not None:
            self.mh_row_scale_ = out["row_scale"].cpu().numpy()
        tot = burn_in + n_keep
        w = min(window_size, tot)
        self.last_acceptance_rate = float(out["acc_count"][tot - w:].sum().item()) / (w * len(data_x))
        print(f"Final MCMC Acceptance Rate: {self.last_acceptance_rate:.4f}")
        if diagnostics:
            self._store_diagnostics(out["draws"], "metropolis_hastings_sampler")
        return out["draws"].cpu().numpy()

    def hmc_sampler(self, data, n_keep=3000, burn_in=5000, step_size=hmc_mod.DEFAULT_STEP_SIZE, n_leapfrog=hmc_mod.DEFAULT_N_LEAPFROG,
                    target_acceptance_rate=hmc_mod.DEFAULT_TARGET, adapt=True, diagnostics=False, mass='identity', partial=False,
                    max_trajectory=None, jitter_leapfrog=False):
        """Posterior samples of Z, shape (n_keep, n, q), by Hamiltonian Monte Carlo on get_log_posterior: ``n_leapfrog`` steps per
        transition, identity mass, one chain per row.  ``adapt=True``: every chain adapts a step size of its own during burn-in
        towards ``target_acceptance_rate``, starting from ``step_size`` (causal_hmc.py); the retained chain is plain HMC.  The steps
        are left in ``self.hmc_row_step_``.  ``mass='diag'`` (needs ``adapt=True``): every chain also estimates a scale per latent
        coordinate from its own burn-in draws, in windows, and keeps it afterwards (a diagonal metric, causal_hmc.py); the scales
        are left in ``self.hmc_row_mass_`` [n, q].  diagnostics=True: as in metropolis_hastings_sampler.  ``partial=True``: NaN in
        ``data_y``, or in ``data_x`` and ``data_y``, marks what a row does not observe; its chain samples p(z | x, v) or p(z | v)
        (``predict_new``).  A row with its outcome observed and its treatment not is refused.  ``max_trajectory`` /
        ``jitter_leapfrog``: as in ``predict(sampler='hmc')``; the mean steps per retained transition are left in
        ``self.hmc_row_leapfrog_``."""
        step_size, n_leapfrog, target = hmc_mod.resolve(type(self).__name__, self._p, step_size, n_leapfrog, target_acceptance_rate, adapt)
        mass = hmc_mod.check_mass(mass, True, adapt, burn_in)
        traj_kw = self._traj_kw(hmc_mod.check_trajectory(max_trajectory, jitter_leapfrog))
        self.hmc_row_step_ = None
        self.hmc_row_mass_ = None
        self.hmc_row_leapfrog_ = None
        data_x, data_y, data_v = data
        if partial:
            hmc_mod.check_partial_rows(np.asarray(data_x, np.float32).reshape(-1), np.asarray(data_y, np.float32).reshape(-1))
        out = self.engine.hmc_sample(self._dev(data_x).reshape(-1), self._dev(data_y).reshape(-1), self._dev(data_v), burn_in, n_keep,
                                     step_size, n_leapfrog, self._next_seed(), want_draws=True, adapt=target, mass=mass, partial=bool(partial),
                                     **traj_kw)
        self.hmc_row_step_ = out["row_step"].cpu().numpy()
        if traj_kw:
            self.hmc_row_leapfrog_ = out["row_leapfrog"].cpu().numpy()
        if mass is not None:
            self.hmc_row_mass_ = out["mass_scale"].cpu().numpy()
        tot = burn_in + n_keep
        w = min(100, tot)
        self.last_acceptance_rate = float(out["acc_count"][tot - w:].sum().item()) / (max(1, w) * len(data_x))
        print(f"Final MCMC Acceptance Rate: {self.last_acceptance_rate:.4f}")
        if diagnostics:
            self._store_diagnostics(out["draws"], "hmc_sampler")
        return out["draws"].cpu().numpy()

    def _store_diagnostics(self, draws_dev, where):
        from .. import diagnostics as dg         # the samplers' `diagnostics` flag shadows the module in their bodies
        self.mcmc_diagnostics_ = dg.chain_diagnostics(draws_dev)
        dg.warn_if_not_mixed(self.mcmc_diagnostics_, self.params, type(self).__name__ + "." + where)

    def infer_from_latent_posterior(self, data_posterior_z, x_values=None, sample_y=True, eps=1e-6, seed=None):
        """Causal effects from posterior draws of Z, shape (n_keep, n, q) (base.py:671-763): binary treatment -> ITE draws
        (n_keep, n); continuous -> ADRF draws (len(x_values), n_keep).  `predict` computes the same quantities inside the
        sampling kernel without materialising the draws; this is the stand-alone form of the reference."""
        draws = self._dev(data_posterior_z)
        if not self._p["binary_treatment"] and x_values is None:
            raise ValueError("For continuous treatment, `x_values` must not be None. Provide a list or numpy array.")
        n = draws.shape[1]
        x0 = torch.zeros(n, device=self.engine.device)          # the treatment slot is overwritten by the counterfactual dose
        out = self.engine.effects(x0, draws, 0, self._next_seed() if seed is None else seed, x_values=x_values, sample_y=sample_y)
        return out.cpu().numpy()

    def get_log_posterior(self, data_x, data_y, data_v, data_z, eps=1e-6):
        """log p(z | x, y, v) + const, shape (n,) (base.py:765-817)."""
        return self.engine.logpost(self._dev(data_x).reshape(-1), self._dev(data_y).reshape(-1), self._dev(data_v),
                                   self._dev(data_z)).cpu().numpy()
