"""Shared inputs and the fp64 autograd oracle of the PPO tests (test_ppo.py, test_gpu_ppo.py)."""
import torch

GAMMA, LAM, CLIP, VCLIP, BC, EC = 0.99, 0.95, 0.1, 0.1, 0.5, 0.01


def recipe(T, B, done_row=None):
    """The V-trace kernel test's inputs (tests/test_gpu_kernels.py) plus a second value array."""
    g = torch.Generator().manual_seed(0)
    lpn = torch.randn(T, B, generator=g) * 0.3 - 5
    lpo = lpn + torch.randn(T, B, generator=g) * 0.2
    v_old = torch.randn(T + 1, B, generator=g)
    v = v_old[:T] + torch.randn(T, B, generator=g) * 0.15
    rew = torch.randn(T, B, generator=g)
    done = torch.rand(T, B, generator=g) < 0.05
    ent = torch.rand(T, B, generator=g) * 3
    if done_row is not None:
        done[done_row] = True
    values = torch.cat([v, v_old[T:]], 0)  # [T+1, B]: the learner's values, bootstrap row kept
    return dict(lpn=lpn, lpo=lpo, v_old=v_old, values=values, rew=rew, done=done, ent=ent)


def autograd_oracle(c, adv, ret, stats, clip=CLIP, value_clip=VCLIP, bc=BC, ec=EC):
    """fp64: total = pg + value - ec * entropy from torch.min / torch.max / clamp, its autograd
    gradients w.r.t. logp_new and the values, and each element's margin to a branch boundary."""
    d = torch.float64
    T = c["lpn"].shape[0]
    lpn = c["lpn"].to(d).requires_grad_(True)
    values = c["values"].to(d).requires_grad_(True)
    v, vo, R = values[:T], c["v_old"].to(d)[:T], ret.to(d)
    a = (adv.to(d) - stats[0].to(d)) * stats[1].to(d)
    ratio = torch.exp(lpn - c["lpo"].to(d))
    pg = -torch.min(ratio * a, ratio.clamp(1 - clip, 1 + clip) * a).mean()
    e1 = (v - R) ** 2
    if value_clip > 0:
        vc = vo + (v - vo).clamp(-value_clip, value_clip)
        e2 = (vc - R) ** 2
        vl = bc * torch.max(e1, e2).mean()
    else:
        vl = bc * e1.mean()
    ent = c["ent"].to(d).mean()
    total = pg + vl - ec * ent
    g_logp, g_values = torch.autograd.grad(total, [lpn, values])
    r = ratio.detach()
    kl = ((r - 1) - (lpn.detach() - c["lpo"].to(d))).mean()
    cf = ((r - 1).abs() > clip).to(d).mean()
    losses = torch.stack([pg.detach(), vl.detach(), ent, total.detach(), r.mean(), kl, cf])
    # margins (relative) to the boundaries where a gradient is discontinuous
    m_ratio = torch.minimum((r - (1 - clip)).abs() / (1 - clip), (r - (1 + clip)).abs() / (1 + clip))
    m_value = torch.full_like(m_ratio, float("inf"))
    if value_clip > 0:
        dv = (v - vo).detach()
        m_value = (dv.abs() - value_clip).abs()
        clipped = dv.abs() > value_clip
        e1d, e2d = e1.detach(), e2.detach()
        m_tie = (e1d - e2d).abs() / torch.maximum(e1d, e2d).clamp_min(1e-300)
        m_value = torch.where(clipped, torch.minimum(m_value, m_tie), m_value)
    return dict(g_logp=g_logp, g_value=g_values, losses=losses, m_ratio=m_ratio, m_value=m_value,
                a_hat=a, ratio=r)
