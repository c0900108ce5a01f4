#!/usr/bin/env python
"""Learner updates only (synthetic engine-shaped batch), for kernel traces / counter passes
without acting kernels in the trace.

    python tools/learner_only.py --batch 8192 --T 64 --steps 2
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="impala_flat")
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--active", type=float, default=0.007,
                    help="fraction of (frame, cell) pairs with a legal action: 0.007 ~ the random-"
                         "init policy's early game, 0.025 ~ a settled training run (6.5 / 256)")
    ap.add_argument("--occupied", type=float, default=None, metavar="MEAN",
                    help="observations like a rollout's: every cell the empty word except about "
                         "MEAN cells per frame with random one-hot words (a settled run has 19.5 "
                         "of 256); default: uniformly random words, every cell non-empty")
    ap.add_argument("--no_abits", action="store_true",
                    help="no active-cell bitmap rows in the batch (the head counts from masks)")
    ap.add_argument("--set", action="append", default=[],
                    help="enc.<attr>=<int> / head.<attr>=<int>: set a variant attribute of the "
                         "HIP encoder / sparse head before the first update (A/B in one process); "
                         "native.<setter>=<int>: call a kernel-library setter")
    ap.add_argument("--lib", default=None, help="variant library dir (tools/variant.py)")
    ap.add_argument("--bwd_occ", type=int, default=0,
                    help="backward workgroups per CU (the GPU actor runtime's cap is 1; 0: none)")
    ap.add_argument("--fwd_occ", type=int, default=0, help="forward workgroups per CU (as --bwd_occ)")
    ap.add_argument("--algo", default="impala", help="impala (V-trace) | ppo")
    ap.add_argument("--ppo_epochs", type=int, default=1,
                    help="--algo ppo: optimiser steps per update (the time printed is per update)")
    ap.add_argument("--ppo_minibatches", type=int, default=1,
                    help="--algo ppo: optimiser steps per epoch, each on T / K rows of the batch")
    ap.add_argument("--ppo_target_kl", type=float, default=0.0,
                    help="--algo ppo: > 0 reads each step's approx_kl on the host (early stop)")
    ap.add_argument("--ppo_adv", default="gae",
                    help="--algo ppo: gae | vtrace (the V-trace(lambda) scan; K > 1: the pre-pass "
                         "scores the actions too)")
    ap.add_argument("--vtrace_lambda", type=float, default=1.0,
                    help="--algo impala: V-trace(lambda); off 1 the objective is mbk_vtrace_upgo")
    ap.add_argument("--upgo_cost", type=float, default=0.0,
                    help="--algo impala: weight of the UPGO term; > 0: mbk_vtrace_upgo")
    ap.add_argument("--upgo_rho_bar", type=float, default=1.0,
                    help="--algo impala: importance-weight bar of the UPGO term")
    a = ap.parse_args()
    import torch

    from tools.variant import use_lib
    use_lib(a.lib)
    if a.bwd_occ or a.fwd_occ:
        from microbeast_amd import _native as N
        N.check(N.kernels().mbk_set_learner_occupancy(a.fwd_occ, a.bwd_occ), "set_learner_occupancy")

    from microbeast_amd.config import parse_flags
    from microbeast_amd.learner import Learner, LearnerHParams
    from microbeast_amd.models.factory import make_model

    dev = torch.device("cuda", 0)
    flags = parse_flags(["--device", "cuda", "--arch", a.arch, "--env_size", str(a.size),
                         "--quiet"], interactive=False)
    torch.manual_seed(0)
    learner = Learner(make_model(flags, dev),
                      LearnerHParams(algo=a.algo, ppo_epochs=a.ppo_epochs,
                                     ppo_minibatches=a.ppo_minibatches,
                                     ppo_target_kl=a.ppo_target_kl, ppo_adv=a.ppo_adv,
                                     vtrace_lambda=a.vtrace_lambda, upgo_cost=a.upgo_cost,
                                     upgo_rho_bar=a.upgo_rho_bar), dev)
    S, T, B = a.size * a.size, a.T, a.batch
    g = torch.Generator(device=dev).manual_seed(1)
    # sparse legal-action masks with --active of the cells live, like the engine's rollouts
    mask = torch.zeros(T + 1, B, S, 3, dtype=torch.int32, device=dev)
    act = torch.rand(T + 1, B, S, device=dev, generator=g) < a.active
    mask[..., 0] = torch.where(act, torch.randint(1, 2 ** 31 - 1, (T + 1, B, S), device=dev,
                                                  generator=g, dtype=torch.int32), 0)
    obs = torch.randint(0, 2 ** 26, (T + 1, B, S), dtype=torch.int32, device=dev, generator=g)
    if a.occupied is not None:
        from microbeast_amd.ops.encoder import EMPTY_WORD, PLANE_GROUPS
        word = torch.zeros(T + 1, B, S, dtype=torch.int32, device=dev)
        for off, k in PLANE_GROUPS:
            word |= 1 << (off + torch.randint(0, k, (T + 1, B, S), dtype=torch.int32, device=dev,
                                              generator=g))
        occ = torch.rand(T + 1, B, S, device=dev, generator=g) < a.occupied / S
        obs = torch.where(occ, word, EMPTY_WORD)
        del word, occ
    batch = {
        "obs": obs,
        "mask": mask,
        "action": torch.zeros(T + 1, B, S, 7, dtype=torch.uint8, device=dev),
        "logp": -torch.rand(T + 1, B, device=dev, generator=g),
        "reward": torch.randn(T + 1, B, device=dev, generator=g),
        "done": torch.zeros(T + 1, B, dtype=torch.uint8, device=dev),
    }
    if not a.no_abits and S % 32 == 0:  # what the fused acting step writes with the rollout
        live = (mask != 0).any(-1).view(T + 1, B, S // 32, 32).to(torch.int64)
        w = (live << torch.arange(32, device=dev)).sum(-1)
        batch["abits"] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    learner.learn(batch)
    for kv in a.set:
        k, v = kv.split("=")
        obj, attr = k.split(".")
        if obj == "native":  # a kernel-library setter: native.mbk_x_set=<int>
            from microbeast_amd import _native as N
            getattr(N.kernels(), attr)(*[int(x) for x in v.split(":")])  # a:b -> two ints
            continue
        m = learner.model
        tgt = m._hip_enc if obj == "enc" else m._head(dev)
        assert hasattr(tgt, attr), kv
        setattr(tgt, attr, type(getattr(tgt, attr))(int(v)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        learner.learn(batch)
    torch.cuda.synchronize()
    print(f"{(time.perf_counter() - t0) / a.steps * 1e3:.3f} ms per update "
          f"({(T * B) / 1e3:.0f}K frames, {learner.last_opt_steps} optimiser steps in the last)",
          flush=True)


if __name__ == "__main__":
    main()
