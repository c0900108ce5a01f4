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
        obs, mask, action = batch["obs"], batch["mask"], batch["action"]
        T1, B = batch["logp"].shape[:2]
        T = T1 - 1
        self.flat.zero_grad()
        self.reducer.start_step()
        flat_obs = obs.reshape(T1 * B, *obs.shape[2:])
        S = mask.shape[2]
        m = mask[:T].reshape(T * B, S, mask.shape[-1])
        a = action[:T].reshape(T * B, S, action.shape[-1])
        kw = {}
        ab = batch.get("abits")
        if ab is not None and getattr(self.model, "accepts_abits", False):
            # the acting step's active-cell bitmap: the head compaction skips the mask pass
            kw["abits"] = ab[:T].reshape(T * B, ab.shape[-1])
        logp, ent, value = self.model.evaluate(flat_obs, m, a, n_score=T * B, **kw)
        if self.hp.vtrace_lambda == 1.0 and self.hp.upgo_cost == 0.0:
            vt = vtrace(logp.view(T, B), batch["logp"][:T], value.view(T1, B), batch["reward"][:T],
                        batch["done"][:T], ent.view(T, B), gamma=self.hp.gamma, rho_bar=self.hp.rho_bar,
                        c_bar=self.hp.c_bar, pg_rho_bar=self.hp.pg_rho_bar,
                        baseline_cost=self.hp.baseline_cost, entropy_cost=self.hp.entropy_cost,
                        reward_clip=self.hp.reward_clip, ws=self.ws)
        else:  # V-trace(lambda) targets and / or the UPGO term: losses [6]
            vt = vtrace_upgo(logp.view(T, B), batch["logp"][:T], value.view(T1, B),
                             batch["reward"][:T], batch["done"][:T], ent.view(T, B),
                             gamma=self.hp.gamma, rho_bar=self.hp.rho_bar, c_bar=self.hp.c_bar,
                             pg_rho_bar=self.hp.pg_rho_bar, baseline_cost=self.hp.baseline_cost,
                             entropy_cost=self.hp.entropy_cost, reward_clip=self.hp.reward_clip,
                             lam=self.hp.vtrace_lambda, upgo_cost=self.hp.upgo_cost,
                             upgo_rho_bar=self.hp.upgo_rho_bar, ws=self.ws)
        self.phases.mark("fwd")
        if sync_timing and logp.is_cuda:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        torch.autograd.backward(
            [logp, value, ent], [vt.g_logp.reshape(-1), vt.g_value.reshape(-1),
                                 self._const_grad(ent, vt.g_ent)])
        if self.flat.adopt_grads() and self.info.enabled:
            raise RuntimeError("a direct-gradient parameter's gradient was not written into "
                               "its flat slot; its all-reduce bucket went out stale")
        self.phases.mark("bwd")
        self.reducer.finish()
        self.phases.mark("allreduce")
        if sync_timing and logp.is_cuda:
            torch.cuda.synchronize()
        t2 = time.perf_counter()
        self.opt.step(grad_scale=self.reducer.grad_scale)
        self.phases.mark("optim")
        if sync_timing and logp.is_cuda:
            torch.cuda.synchronize()
        t3 = time.perf_counter()
        self.n_updates += 1
        self.last_opt_steps = 1
        self.timing = {"fwd_s": t1 - t0, "bwd_allreduce_s": t2 - t1, "optim_s": t3 - t2}
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
        t_fwd = t_bwd = t_opt = 0.0
        self.phases.start()
        obs, mask, action = batch["obs"], batch["mask"], batch["action"]
        T1, B = batch["logp"].shape[:2]
        T = T1 - 1
        flat_obs = obs.reshape(T1 * B, *obs.shape[2:])
        S = mask.shape[2]
        m = mask[:T].reshape(T * B, S, mask.shape[-1])
        a = action[:T].reshape(T * B, S, action.shape[-1])
        kw = {}
        ab = batch.get("abits")
        if ab is not None and getattr(self.model, "accepts_abits", False):
            kw["abits"] = ab[:T].reshape(T * B, ab.shape[-1])
        cuda = batch["logp"].is_cuda
        g = v_old = None
        for epoch in range(hp.ppo_epochs):
            t0 = time.perf_counter()
            self.flat.zero_grad()
            self.reducer.start_step()
            logp, ent, value = self.model.evaluate(flat_obs, m, a, n_score=T * B, **kw)
            if epoch == 0 and hp.ppo_adv == "vtrace":
                v_old, g = self._vtrace_adv(batch, value, logp, T1, B, cuda)
            elif epoch == 0:
                if cuda:  # (a workspace buffer: the forward's own output is rewritten per epoch)
                    v_old = self.ws.get("ppo_v_old", (T1, B), value.device)
                    v_old.copy_(value.detach().view(T1, B))
                else:
                    v_old = value.detach().float().view(T1, B).clone()
                g = gae(v_old, batch["reward"][:T], batch["done"][:T], gamma=hp.gamma,
                        lam=hp.gae_lambda, reward_clip=hp.reward_clip, norm_adv=hp.ppo_norm_adv,
                        ws=self.ws)
            out = ppo_loss(logp.view(T, B), batch["logp"][:T], value.view(T1, B), v_old, g.adv,
                           g.ret, g.stats, ent.view(T, B), clip=hp.ppo_clip,
                           value_clip=hp.ppo_value_clip, baseline_cost=hp.baseline_cost,
                           entropy_cost=hp.entropy_cost, ws=self.ws)
            self.phases.mark("fwd")
            if sync_timing and cuda:
                torch.cuda.synchronize()
            t1 = time.perf_counter()
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
            t3 = time.perf_counter()
            t_fwd, t_bwd, t_opt = t_fwd + t1 - t0, t_bwd + t2 - t1, t_opt + t3 - t2
        self.n_updates += 1
        self.last_opt_steps = hp.ppo_epochs
        self.timing = {"fwd_s": t_fwd, "bwd_allreduce_s": t_bwd, "optim_s": t_opt}
        return out.losses

    def _learn_ppo_steps(self, batch: dict, sync_timing: bool = False) -> torch.Tensor:
        """``_learn_ppo`` with ``ppo_minibatches`` K > 1 and / or ``ppo_target_kl`` > 0.

        K > 1: one no-grad value pass over the slot gives ``v_old`` for GAE (once per rollout)
        and one launch gives each block's own advantage statistics; every epoch then visits its
        K blocks of T / K consecutive rows (all envs) once, in ``ppo_block_order``'s order, and
        each visit is a full optimiser step on that block alone: zero grads -> forward on the
        block's rows (no bootstrap row) -> block loss -> backward -> all-reduce -> Adam. K == 1
        keeps ``_learn_ppo``'s steps (epoch 0's own values are ``v_old``). ``ppo_adv="vtrace"``:
        the pre-pass is a no-grad ``evaluate`` over the slot, whose log-probs the V-trace(lambda)
        scan needs beside the values (``_vtrace_adv``).

        ``ppo_target_kl`` > 0: the host reads a step's approx_kl only AFTER that step's
        backward, all-reduce and Adam are queued (an event recorded behind the loss launch and
        a 4-byte copy into pinned memory), so the GPU never idles on the read; a step whose
        approx_kl (the MAX over ranks, one float on the host group) exceeds the target is
        still applied and is the rollout's last. Returns the device tensor [7]: K > 1: the mean
        over the steps of the last epoch entered; K == 1: the last step's."""
        hp = self.hp
        K = hp.ppo_minibatches
        t_fwd = t_bwd = t_opt = 0.0
        self.phases.start()
        obs, mask, action = batch["obs"], batch["mask"], batch["action"]
        T1, B = batch["logp"].shape[:2]
        T = T1 - 1
        if T % K != 0:
            raise ValueError(f"--ppo_minibatches {K} does not divide the unroll length {T}")
        Tm = T // K
        S = mask.shape[2]
        ab = batch.get("abits")
        if ab is not None and not getattr(self.model, "accepts_abits", False):
            ab = None

        def rows(t0, t1, n_val):
            """evaluate()'s arguments for rows [t0, t1) scored, values on [t0, t0 + n_val)"""
            kw = {} if ab is None else {"abits": ab[t0:t1].reshape((t1 - t0) * B, ab.shape[-1])}
            return (obs[t0:t0 + n_val].reshape(n_val * B, *obs.shape[2:]),
                    mask[t0:t1].reshape((t1 - t0) * B, S, mask.shape[-1]),
                    action[t0:t1].reshape((t1 - t0) * B, S, action.shape[-1])), kw

        cuda = batch["logp"].is_cuda
        g = v_old = stats = mean = None
        if K > 1:
            args, kw = rows(0, T, T1)
            if hp.ppo_adv == "vtrace":  # the scan needs the pass's log-probs too
                with torch.no_grad():
                    lp, _, v = self.model.evaluate(*args, n_score=T * B, **kw)
                v_old, g = self._vtrace_adv(batch, v, lp, T1, B, cuda)
            else:
                with torch.no_grad():
                    if hasattr(self.model, "values"):
                        v = self.model.values(args[0])
                    else:
                        v = self.model.evaluate(*args, n_score=T * B, **kw)[2]
                v_old = self._snapshot_values(v, T1, B, cuda)
                g = gae(v_old, batch["reward"][:T], batch["done"][:T], gamma=hp.gamma,
                        lam=hp.gae_lambda, reward_clip=hp.reward_clip,
                        norm_adv=hp.ppo_norm_adv, ws=self.ws)
            stats = adv_stats_rows(g.adv, K, hp.ppo_norm_adv, ws=self.ws)
        steps, stop = 0, False
        for epoch in range(hp.ppo_epochs):
            order = ppo_block_order(hp.ppo_seed, self.n_updates, epoch, K, hp.ppo_shuffle)
            for j, k in enumerate(order):
                t0 = time.perf_counter()
                self.flat.zero_grad()
                self.reducer.start_step()
                if K == 1:
                    args, kw = rows(0, T, T1)
                    logp, ent, value = self.model.evaluate(*args, n_score=T * B, **kw)
                    if epoch == 0 and hp.ppo_adv == "vtrace":
                        v_old, g = self._vtrace_adv(batch, value, logp, T1, B, cuda)
                    elif epoch == 0:
                        v_old = self._snapshot_values(value, T1, B, cuda)
                        g = gae(v_old, batch["reward"][:T], batch["done"][:T], gamma=hp.gamma,
                                lam=hp.gae_lambda, reward_clip=hp.reward_clip,
                                norm_adv=hp.ppo_norm_adv, ws=self.ws)
                    out = ppo_loss(logp.view(T, B), batch["logp"][:T], value.view(T1, B), v_old,
                                   g.adv, g.ret, g.stats, ent.view(T, B), clip=hp.ppo_clip,
                                   value_clip=hp.ppo_value_clip, baseline_cost=hp.baseline_cost,
                                   entropy_cost=hp.entropy_cost, ws=self.ws)
                    mean = out.losses
                else:
                    r0 = k * Tm
                    args, kw = rows(r0, r0 + Tm, Tm)
                    logp, ent, value = self.model.evaluate(*args, n_score=Tm * B, **kw)
                    out = ppo_loss_rows(logp.view(Tm, B), batch["logp"][:T], value.view(Tm, B),
                                        v_old, g.adv, g.ret, stats[k], r0, ent.view(Tm, B),
                                        clip=hp.ppo_clip, value_clip=hp.ppo_value_clip,
                                        baseline_cost=hp.baseline_cost,
                                        entropy_cost=hp.entropy_cost, step=j, epoch_mean=mean,
                                        ws=self.ws)
                    mean = out.epoch_mean
                kl_ev = self._kl_record(out.losses) if hp.ppo_target_kl > 0 else None
                self.phases.mark("fwd")
                if sync_timing and cuda:
                    torch.cuda.synchronize()
                t1 = time.perf_counter()
                torch.autograd.backward(
                    [logp, value, ent], [out.g_logp.reshape(-1), out.g_value.reshape(-1),
                                         self._const_grad(ent, out.g_ent)])
                if self.flat.adopt_grads() and self.info.enabled:
                    raise RuntimeError("a direct-gradient parameter's gradient was not written "
                                       "into its flat slot; its all-reduce bucket went out stale")
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
                t3 = time.perf_counter()
                t_fwd, t_bwd, t_opt = t_fwd + t1 - t0, t_bwd + t2 - t1, t_opt + t3 - t2
                steps += 1
                # the step above is queued (and applied) whatever its KL says
                if hp.ppo_target_kl > 0 and self._kl_read(out.losses, kl_ev) > hp.ppo_target_kl:
                    stop = True
                    break
            if stop:
                break
        self.n_updates += 1
        self.last_opt_steps = steps
        self.timing = {"fwd_s": t_fwd, "bwd_allreduce_s": t_bwd, "optim_s": t_opt}
        return mean

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
