"""IMPALA learner step: forward -> V-trace -> backward -> all-reduce -> Adam (``algo="ppo"``:
the PPO objective in its place, ``Learner._learn_ppo``).

Reference: ``PPO_learn`` (libs/utils.py:223-342) + the learner loop
(microbeast.py:211-248). Re-designed:

* the batch is time-major ``[T+1, B, ...]`` and stays that way (no
  reshape scrambling); row t holds obs_t/mask_t with the action
  a_t sampled there (D3 fixed);
* one model, one optimizer over a flat fp32 buffer (D1 fixed);
* the V-trace kernel returns dL/dlogp, dL/dV, dL/dH directly and backward is
  seeded with them (``autograd.backward`` on three outputs) — no scalar
  loss graph, no extra reductions;
* gradients are all-reduced in buckets overlapped with backward (DP);
* nothing syncs the host inside ``learn`` except the optional loss readout (and PPO's
  target-KL stop, whose one-float read waits behind the step it follows:
  ``Learner._learn_ppo_steps``).

The three entry points (``learn``, ``_learn_ppo``, ``_learn_ppo_steps``) share one copy of each
piece: ``Rollout.rows`` slices the slot into ``evaluate()``'s arguments, ``_objective_kw`` builds
the objective's keyword arguments from the hyper-parameters, ``_ppo_targets`` turns a first
pass into (v_old, advantages), ``_ppo_full_step`` is the full-batch PPO step up to its loss, and
``_fwd_done`` + ``_step_tail`` are every optimiser step from the "fwd" mark to the "optim" mark.
"""
from __future__ import annotations

import time
from dataclasses import dataclass

import torch

from .ops.copy import full, multi_copy
from .ops.optim import FlatAdam, FlatParams
from .ops.ppo import adv_stats_rows, gae, ppo_loss, ppo_loss_rows, vtrace_adv
from .ops.vtrace import VTraceWorkspace, vtrace, vtrace_upgo
from .parallel.dist import DistInfo, GradAllReducer, broadcast_flat, host_max
from .utils.metrics import PhaseTimer


@dataclass
class LearnerHParams:
    lr: float = 2.5e-4          # microbeast.py:200
    adam_eps: float = 1e-5      # microbeast.py:200
    gamma: float = 0.99         # microbeast.py:118 / libs/utils.py:277
    baseline_cost: float = 0.5  # libs/utils.py:323 (0.5 * mean sq)
    entropy_cost: float = 0.01  # libs/utils.py:329
    rho_bar: float = 1.0        # libs/utils.py:293
    c_bar: float = 1.0          # libs/utils.py:294
    pg_rho_bar: float = 1.0     # libs/utils.py:316
    reward_clip: float = 0.0    # reference: none
    max_grad_norm: float = 0.0  # reference: none
    bucket_mb: float = 8.0
    allreduce_dtype: str = "fp32"  # fp32 | bf16 (gradient all-reduce payload)
    comm_rehearsal: bool = False   # world 1: stand-in collectives on a 4th stream (dist.py)
    algo: str = "impala"           # impala (V-trace) | ppo (ops/ppo.py)
    gae_lambda: float = 0.95       # ppo: GAE lambda
    ppo_clip: float = 0.1          # ppo: ratio clip eps
    ppo_value_clip: float = 0.1    # ppo: value clip eps_v (0: unclipped value loss)
    ppo_epochs: int = 1            # ppo: passes over the rollout (epochs)
    ppo_norm_adv: bool = True      # ppo: normalise the advantages over the rank's batch
    ppo_minibatches: int = 1       # ppo: K optimiser steps per epoch, each on T / K rows
    ppo_shuffle: bool = True       # ppo: visit the K row blocks in a fresh order each epoch
    ppo_target_kl: float = 0.0     # ppo: > 0 ends the rollout's steps after one exceeds it
    ppo_seed: int = 0              # ppo: seeds the block orders (with n_updates and the epoch)
    ppo_adv: str = "gae"           # ppo: gae | vtrace (rho_bar / c_bar-clipped, ops/ppo.py)
    vtrace_lambda: float = 1.0     # impala: V-trace(lambda), the trace cut by lambda min(c_bar, w)
    upgo_cost: float = 0.0         # impala: weight of the UPGO policy term (0: off)
    upgo_rho_bar: float = 1.0      # impala: importance-weight bar of the UPGO term

    def __post_init__(self):
        if self.algo not in ("impala", "ppo"):
            raise ValueError(f"--algo {self.algo!r}: expected impala | ppo")
        if not 0.0 <= self.vtrace_lambda <= 1.0:
            raise ValueError(f"--vtrace_lambda {self.vtrace_lambda}: expected 0 <= lambda <= 1")
        if not self.upgo_cost >= 0:
            raise ValueError(f"--upgo_cost {self.upgo_cost}: expected >= 0 (0 = off)")
        if not self.upgo_rho_bar > 0:
            raise ValueError(f"--upgo_rho_bar {self.upgo_rho_bar}: expected > 0")
        if self.algo == "ppo" and (self.upgo_cost > 0 or self.vtrace_lambda != 1.0):
            raise ValueError(f"--algo ppo: --upgo_cost {self.upgo_cost} / --vtrace_lambda "
                             f"{self.vtrace_lambda} act on the IMPALA objective only (PPO's trace "
                             "is cut by --gae_lambda)")
        if self.ppo_adv not in ("gae", "vtrace"):
            raise ValueError(f"--ppo_adv {self.ppo_adv!r}: expected gae | vtrace")
        if self.ppo_adv == "vtrace" and not (self.rho_bar > 0 and self.c_bar > 0):
            raise ValueError(f"--ppo_adv vtrace: --rho_bar {self.rho_bar} / --c_bar {self.c_bar}: "
                             "expected > 0")
        if self.ppo_epochs < 1:
            raise ValueError(f"--ppo_epochs {self.ppo_epochs}: expected >= 1")
        if self.ppo_minibatches < 1:
            raise ValueError(f"--ppo_minibatches {self.ppo_minibatches}: expected >= 1")
        if not self.ppo_target_kl >= 0:
            raise ValueError(f"--ppo_target_kl {self.ppo_target_kl}: expected >= 0 (0 = off)")


def ppo_block_order(seed: int, n_updates: int, epoch: int, K: int, shuffle: bool = True) -> list:
    """The order in which epoch ``epoch`` of rollout ``n_updates`` visits its K row blocks: a
    permutation from a CPU generator seeded from (seed, n_updates, epoch), so a resumed run
    repeats it with no generator state in the checkpoint and no RNG of the process or the
    device is touched. ``shuffle`` off: 0..K-1."""
    if not shuffle or K == 1:
        return list(range(K))
    g = torch.Generator()
    g.manual_seed(((int(seed) * 1_000_003 + int(n_updates)) * 1_000_003 + int(epoch))
                  % (2 ** 63 - 1))
    return torch.randperm(K, generator=g).tolist()


class Rollout:
    """One batch as ``evaluate()`` takes it: ``rows`` hands out slices and reshapes of the
    slot's own arrays (views, no copy). ``abits``, the acting step's active-cell bitmap with
    which the head compaction skips the mask pass, is dropped here when the model does not
    accept it."""

    def __init__(self, batch: dict, model: torch.nn.Module):
        self.batch = batch
        self.obs, self.mask, self.action = batch["obs"], batch["mask"], batch["action"]
        ab = batch.get("abits")
        self.abits = ab if ab is not None and getattr(model, "accepts_abits", False) else None
        T1, self.B = batch["logp"].shape[:2]
        self.T = T1 - 1
        self.cuda = batch["logp"].is_cuda

    def rows(self, t0: int, t1: int, n_val: int):
        """evaluate()'s arguments for rows [t0, t1) scored, values on [t0, t0 + n_val)"""
        obs, mask, action, ab = self.obs, self.mask, self.action, self.abits
        n = (t1 - t0) * self.B
        kw = {} if ab is None else {"abits": ab[t0:t1].reshape(n, ab.shape[-1])}
        return (obs[t0:t0 + n_val].reshape(n_val * self.B, *obs.shape[2:]),
                mask[t0:t1].reshape(n, mask.shape[2], mask.shape[-1]),
                action[t0:t1].reshape(n, mask.shape[2], action.shape[-1])), kw


class Learner:
    def __init__(self, model: torch.nn.Module, hp: LearnerHParams, device: torch.device,
                 info: DistInfo | None = None):
        self.model = model.to(device)
        self.device = device
        self.hp = hp
        self.info = info or DistInfo()
        self.flat = FlatParams(self.model, device)
        broadcast_flat(self.flat, self.info)
        self.opt = FlatAdam(self.flat, lr=hp.lr, eps=hp.adam_eps, max_grad_norm=hp.max_grad_norm)
        self.reducer = GradAllReducer(
            self.flat, self.info, hp.bucket_mb,
            torch.bfloat16 if hp.allreduce_dtype == "bf16" else torch.float32,
            rehearse=hp.comm_rehearsal)
        self.ws = VTraceWorkspace()
        self.n_updates = 0
        self.last_opt_steps = 0  # optimiser steps applied in the last learn()
        # ppo_adv="vtrace": device tensor [3] = mean importance weight, share above rho_bar,
        # share above c_bar of the last rollout (ops/ppo.py)
        self.last_is_stats = None
        self.timing = {}
        # HIP-event split fwd / bwd / allreduce(wait) / optim (+ publish marked by the
        # caller), read one update late without a host sync
        self.phases = PhaseTimer(enabled=device.type == "cuda")

    def learn(self, batch: dict, sync_timing: bool = False) -> torch.Tensor:
        """batch keys (time-major): obs [T+1,B,...], mask [T+1,B,S,3] int32,
        action [T+1,B,S,7] uint8, logp [T+1,B], reward [T+1,B], done [T+1,B].
        Returns the device tensor [5] = pg, value, entropy, total, mean rho (``algo="ppo"``:
        [7], see ``_learn_ppo``; ``vtrace_lambda`` < 1 or ``upgo_cost`` > 0: [6], + the
        unweighted UPGO loss, from ``ops.vtrace.vtrace_upgo`` in ``vtrace``'s place)."""
        if self.hp.algo == "ppo":
            return self._learn_ppo(batch, sync_timing)
        t0 = time.perf_counter()
        self.phases.start()
        ro = Rollout(batch, self.model)
        T, B = ro.T, ro.B
        self.flat.zero_grad()
        self.reducer.start_step()
        args, kw = ro.rows(0, T, T + 1)
        logp, ent, value = self.model.evaluate(*args, n_score=T * B, **kw)
        # V-trace(lambda) targets and / or the UPGO term: vtrace_upgo, losses [6]
        upgo = self.hp.vtrace_lambda != 1.0 or self.hp.upgo_cost != 0.0
        vt = (vtrace_upgo if upgo else vtrace)(
            logp.view(T, B), batch["logp"][:T], value.view(T + 1, B), batch["reward"][:T],
            batch["done"][:T], ent.view(T, B), ws=self.ws, **self._objective_kw(upgo))
        t1 = self._fwd_done(sync_timing, ro.cuda)
        t2, t3 = self._step_tail(logp, value, ent, vt, sync_timing, ro.cuda)
        self._rollout_done(1, [t1 - t0, t2 - t1, t3 - t2])
        return vt.losses

    def _learn_ppo(self, batch: dict, sync_timing: bool = False) -> torch.Tensor:
        """``ppo_epochs`` full-batch epochs on one rollout: each is zero grads -> forward ->
        clipped losses -> backward -> all-reduce -> Adam, so Adam's step count advances once
        per epoch while ``n_updates`` counts rollouts. Epoch 0 snapshots its own values as
        ``v_old`` and runs GAE on them (ops/ppo.py); later epochs reuse adv / ret / stats /
        v_old from the workspace. ``ppo_adv="vtrace"``: epoch 0 snapshots its own log-probs as
        well and runs the V-trace(lambda) scan in GAE's place (``_vtrace_adv``), for rollouts
        acted by lagged weights. Under data parallelism the advantages are normalised with
        each rank's own statistics. Returns the last epoch's device tensor [7] = pg, value,
        entropy, total, mean ratio, approx_kl, clip_frac; nothing syncs the host.
        ``ppo_minibatches`` > 1 or ``ppo_target_kl`` > 0: ``_learn_ppo_steps`` instead."""
        hp = self.hp
        if hp.ppo_minibatches > 1 or hp.ppo_target_kl > 0:
            return self._learn_ppo_steps(batch, sync_timing)
        times = [0.0, 0.0, 0.0]
        self.phases.start()
        ro = Rollout(batch, self.model)
        targets = None
        for _ in range(hp.ppo_epochs):
            t0 = self._step_begin()
            logp, ent, value, out, targets = self._ppo_full_step(ro, targets)
            t1 = self._fwd_done(sync_timing, ro.cuda)
            t2, t3 = self._step_tail(logp, value, ent, out, sync_timing, ro.cuda)
            times = [times[0] + t1 - t0, times[1] + t2 - t1, times[2] + t3 - t2]
        self._rollout_done(hp.ppo_epochs, times)
        return out.losses

    def _learn_ppo_steps(self, batch: dict, sync_timing: bool = False) -> torch.Tensor:
        """``_learn_ppo`` with ``ppo_minibatches`` K > 1 and / or ``ppo_target_kl`` > 0.

        K > 1: one no-grad value pass over the slot gives ``v_old`` for GAE (once per rollout)
        and one launch gives each block's own advantage statistics; every epoch then visits its
        K blocks of T / K consecutive rows (all envs) once, in ``ppo_block_order``'s order, and
        each visit is a full optimiser step on that block alone: zero grads -> forward on the
        block's rows (no bootstrap row) -> block loss -> backward -> all-reduce -> Adam. K == 1
        keeps ``_learn_ppo``'s steps (``_ppo_full_step``: epoch 0's own values are ``v_old``).
        ``ppo_adv="vtrace"``: the pre-pass is a no-grad ``evaluate`` over the slot, whose
        log-probs the V-trace(lambda) scan needs beside the values (``_vtrace_adv``).

        ``ppo_target_kl`` > 0: the host reads a step's approx_kl only AFTER that step's
        backward, all-reduce and Adam are queued (an event recorded behind the loss launch and
        a 4-byte copy into pinned memory), so the GPU never idles on the read; a step whose
        approx_kl (the MAX over ranks, one float on the host group) exceeds the target is
        still applied and is the rollout's last. Returns the device tensor [7]: K > 1: the mean
        over the steps of the last epoch entered; K == 1: the last step's."""
        hp = self.hp
        K = hp.ppo_minibatches
        times = [0.0, 0.0, 0.0]
        self.phases.start()
        ro = Rollout(batch, self.model)
        T, B = ro.T, ro.B
        if T % K != 0:
            raise ValueError(f"--ppo_minibatches {K} does not divide the unroll length {T}")
        Tm = T // K
        targets = stats = mean = None
        if K > 1:
            args, kw = ro.rows(0, T, T + 1)
            with torch.no_grad():
                if hp.ppo_adv != "vtrace" and hasattr(self.model, "values"):
                    lp, v = None, self.model.values(args[0])
                else:  # (the V-trace scan needs the pass's log-probs too)
                    lp, _, v = self.model.evaluate(*args, n_score=T * B, **kw)
            targets = self._ppo_targets(ro, v, lp)
            stats = adv_stats_rows(targets[1].adv, K, hp.ppo_norm_adv, ws=self.ws)
        steps, stop = 0, False
        for epoch in range(hp.ppo_epochs):
            order = ppo_block_order(hp.ppo_seed, self.n_updates, epoch, K, hp.ppo_shuffle)
            for j, k in enumerate(order):
                t0 = self._step_begin()
                if K == 1:
                    logp, ent, value, out, targets = self._ppo_full_step(ro, targets)
                    mean = out.losses
                else:
                    r0, (v_old, g) = k * Tm, targets
                    args, kw = ro.rows(r0, r0 + Tm, Tm)
                    logp, ent, value = self.model.evaluate(*args, n_score=Tm * B, **kw)
                    out = ppo_loss_rows(logp.view(Tm, B), batch["logp"][:T], value.view(Tm, B),
                                        v_old, g.adv, g.ret, stats[k], r0, ent.view(Tm, B),
                                        step=j, epoch_mean=mean, ws=self.ws,
                                        **self._objective_kw())
                    mean = out.epoch_mean
                kl_ev = self._kl_record(out.losses) if hp.ppo_target_kl > 0 else None
                t1 = self._fwd_done(sync_timing, ro.cuda)
                t2, t3 = self._step_tail(logp, value, ent, out, sync_timing, ro.cuda)
                times = [times[0] + t1 - t0, times[1] + t2 - t1, times[2] + t3 - t2]
                steps += 1
                # the step above is queued (and applied) whatever its KL says
                if hp.ppo_target_kl > 0 and self._kl_read(out.losses, kl_ev) > hp.ppo_target_kl:
                    stop = True
                    break
            if stop:
                break
        self._rollout_done(steps, times)
        return mean

    def _objective_kw(self, upgo: bool = False) -> dict:
        """The objective's keyword arguments, plain floats from ``hp``: ``ppo_loss`` /
        ``ppo_loss_rows``'s under ``algo="ppo"``, else ``vtrace``'s (``upgo``: those of
        ``vtrace_upgo``)."""
        hp = self.hp
        if hp.algo == "ppo":
            return dict(clip=hp.ppo_clip, value_clip=hp.ppo_value_clip,
                        baseline_cost=hp.baseline_cost, entropy_cost=hp.entropy_cost)
        kw = dict(gamma=hp.gamma, rho_bar=hp.rho_bar, c_bar=hp.c_bar, pg_rho_bar=hp.pg_rho_bar,
                  baseline_cost=hp.baseline_cost, entropy_cost=hp.entropy_cost,
                  reward_clip=hp.reward_clip)
        if upgo:
            kw.update(lam=hp.vtrace_lambda, upgo_cost=hp.upgo_cost, upgo_rho_bar=hp.upgo_rho_bar)
        return kw

    def _step_begin(self) -> float:
        """the head of one PPO optimiser step; returns its host start time"""
        t0 = time.perf_counter()
        self.flat.zero_grad()
        self.reducer.start_step()
        return t0

    def _fwd_done(self, sync_timing: bool, cuda: bool) -> float:
        """behind the loss launch (and ``_kl_record``): the "fwd" mark and the host time t1"""
        self.phases.mark("fwd")
        if sync_timing and cuda:
            torch.cuda.synchronize()
        return time.perf_counter()

    def _step_tail(self, logp, value, ent, out, sync_timing: bool, cuda: bool):
        """The rest of every optimiser step, behind ``_fwd_done``: backward seeded with the
        objective's gradients (``out.g_logp`` / ``g_value`` / the constant ``g_ent``) ->
        all-reduce -> Adam. Returns the host times (t2, t3) after the all-reduce and after Adam."""
        torch.autograd.backward(
            [logp, value, ent], [out.g_logp.reshape(-1), out.g_value.reshape(-1),
                                 self._const_grad(ent, out.g_ent)])
        if self.flat.adopt_grads() and self.info.enabled:
            raise RuntimeError("a direct-gradient parameter's gradient was not written into "
                               "its flat slot; its all-reduce bucket went out stale")
        self.phases.mark("bwd")
        self.reducer.finish()
        self.phases.mark("allreduce")
        if sync_timing and cuda:
            torch.cuda.synchronize()
        t2 = time.perf_counter()
        self.opt.step(grad_scale=self.reducer.grad_scale)
        self.phases.mark("optim")
        if sync_timing and cuda:
            torch.cuda.synchronize()
        return t2, time.perf_counter()

    def _rollout_done(self, steps: int, times: list) -> None:
        """one ``learn`` call's bookkeeping; ``times``: host seconds in fwd, bwd + all-reduce,
        Adam"""
        self.n_updates += 1
        self.last_opt_steps = steps
        self.timing = dict(zip(("fwd_s", "bwd_allreduce_s", "optim_s"), times))

    def _ppo_full_step(self, ro: Rollout, targets):
        """One full-batch PPO step up to its loss: forward on the whole rollout, the rollout's
        targets from this pass where there are none yet (epoch 0), ``ppo_loss``. Returns
        (logp, ent, value, out, targets)."""
        T, B, batch = ro.T, ro.B, ro.batch
        args, kw = ro.rows(0, T, T + 1)
        logp, ent, value = self.model.evaluate(*args, n_score=T * B, **kw)
        if targets is None:
            targets = self._ppo_targets(ro, value, logp)
        v_old, g = targets
        out = ppo_loss(logp.view(T, B), batch["logp"][:T], value.view(T + 1, B), v_old, g.adv,
                       g.ret, g.stats, ent.view(T, B), ws=self.ws, **self._objective_kw())
        return logp, ent, value, out, targets

    def _ppo_targets(self, ro: Rollout, value: torch.Tensor, logp):
        """The rollout's (v_old, GaeOut) from its first pass's values [(T+1) B] and log-probs
        (``ppo_adv="gae"`` reads none: None will do): the V-trace(lambda) scan, or a value
        snapshot and GAE."""
        hp, T, batch = self.hp, ro.T, ro.batch
        if hp.ppo_adv == "vtrace":
            return self._vtrace_adv(batch, value, logp, T + 1, ro.B, ro.cuda)
        v_old = self._snapshot_values(value, T + 1, ro.B, ro.cuda)
        return v_old, gae(v_old, batch["reward"][:T], batch["done"][:T], gamma=hp.gamma,
                          lam=hp.gae_lambda, reward_clip=hp.reward_clip,
                          norm_adv=hp.ppo_norm_adv, ws=self.ws)

    def _snapshot_values(self, value: torch.Tensor, T1: int, B: int, cuda: bool) -> torch.Tensor:
        """detached fp32 [T1, B] copy of a forward's values (on a GPU: a workspace buffer)"""
        if cuda:
            v_old = self.ws.get("ppo_v_old", (T1, B), value.device)
            v_old.copy_(value.detach().view(T1, B))
            return v_old
        return value.detach().float().view(T1, B).clone()

    def _vtrace_adv(self, batch: dict, value: torch.Tensor, logp: torch.Tensor, T1: int, B: int,
                    cuda: bool):
        """``ppo_adv="vtrace"``: snapshot one pass's values [T1, B] and log-probs [T, B] (on a
        GPU: workspace buffers filled by one copy launch) and run the V-trace(lambda) scan on
        them against the batch's behaviour log-probs. Returns (v_old, GaeOut); keeps the
        importance statistics as ``last_is_stats``."""
        hp, T = self.hp, T1 - 1
        if cuda:
            v_old = self.ws.get("ppo_v_old", (T1, B), value.device)
            logp_pi = self.ws.get("ppo_logp_pi", (T, B), value.device)
            multi_copy([(value.detach().float().contiguous(), v_old),
                        (logp.detach().float().contiguous(), logp_pi)])
        else:
            v_old = value.detach().float().view(T1, B).clone()
            logp_pi = logp.detach().float().view(T, B).clone()
        g, self.last_is_stats = vtrace_adv(
            logp_pi, batch["logp"][:T], v_old, batch["reward"][:T], batch["done"][:T],
            gamma=hp.gamma, lam=hp.gae_lambda, rho_bar=hp.rho_bar, c_bar=hp.c_bar,
            reward_clip=hp.reward_clip, norm_adv=hp.ppo_norm_adv, ws=self.ws)
        return v_old, g

    def _kl_record(self, losses: torch.Tensor):
        """Right behind a step's loss launch: queue the 4-byte copy of its approx_kl into pinned
        memory and an event after it (CPU: nothing to queue)."""
        if not losses.is_cuda:
            return None
        if getattr(self, "_kl_host", None) is None:
            self._kl_host = torch.zeros(1, dtype=torch.float32, pin_memory=True)
        # (one float is enough: it is read before the next step's copy is queued)
        self._kl_host.copy_(losses[5:6], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def _kl_read(self, losses: torch.Tensor, ev) -> float:
        """The step's approx_kl on the host, MAX over the data-parallel ranks so that every
        rank stops after the same step."""
        if ev is None:
            kl = float(losses[5])
        else:
            ev.synchronize()
            kl = float(self._kl_host[0])
        return host_max(kl, self.info)
    def _const_grad(self, like: torch.Tensor, value: float) -> torch.Tensor:
        """constant seed gradient (entropy term), filled once per shape / value"""
        c = getattr(self, "_cg", None)
        if c is None or c[0] != (like.shape, like.device, value):
            c = ((like.shape, like.device, value), full(like.shape, value, like.dtype, like.device))
            self._cg = c
        return c[1]

    def state_dict(self):
        return {"model": self.model.state_dict(), "optim": self.opt.state_dict(),
                "n_updates": self.n_updates}

    def load_state_dict(self, sd):
        self.model.load_state_dict(sd["model"])
        self.opt.load_state_dict(sd["optim"])
        self.n_updates = int(sd.get("n_updates", 0))
