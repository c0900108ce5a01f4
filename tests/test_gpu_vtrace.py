"""vtrace.hip on the MI355X against the fp64 oracle (objective_cases.vtrace_oracle64) across its
flags and edges: three different bars, gamma, both costs, the reward clip, no entropy, shapes
from one lane to 66 partial rows (the finalize kernel's strided loop), a done row, all dones;
``want_targets`` off bit-equal to on, poisoned workspaces, bit reproducibility. Tolerances are
those of test_gpu_kernels.py::test_vtrace_kernel_vs_torch; no element is left out."""
import pytest
import torch

from microbeast_amd.ops.vtrace import VTraceWorkspace, vtrace
from objective_cases import DEFAULTS, NONDEFAULT, vtrace_oracle64, vtrace_recipe

pytestmark = pytest.mark.gpu

SHAPES = {
    "37x300": (37, 300, None, False),
    "1x1": (1, 1, None, False),
    "64x257": (64, 257, None, False),      # one lane in the second block
    "5x63": (5, 63, None, False),          # less than one wave
    "3x16641": (3, 16641, None, False),    # 66 partial rows: the finalize kernel loops
    "37x300-done-row": (37, 300, 11, False),
    "9x300-all-done": (9, 300, None, True),  # every vs_t = v_t + rho_t (r_t - v_t)
}
SETTINGS = {
    "defaults": (dict(), True),
    "nondefault": (NONDEFAULT, True),
    "reward-clip": (dict(reward_clip=0.5), True),
    "no-entropy": (dict(), False),
}


def _case(shape):
    T, B, done_row, all_done = SHAPES[shape]
    c = vtrace_recipe(T, B, 0, done_row)
    if all_done:
        c["done"] = torch.ones_like(c["done"])
    return c


def _run(c, dev, ws, kw, use_ent=True, want_targets=True):
    """One kernel call with the partial rows and the bootstrap gradient row poisoned first."""
    T, B = c["lpn"].shape
    nan = float("nan")
    ws.get("partials", (((B + 255) // 256) * 4,), dev).fill_(nan)
    ws.get("g_value", (T + 1, B), dev).fill_(nan)
    ws.get("losses", (5,), dev).fill_(nan)
    d = {k: v.to(dev) for k, v in c.items()}
    return vtrace(d["lpn"], d["lpo"], d["val"], d["rew"], d["done"],
                  d["ent"] if use_ent else None, want_targets=want_targets, ws=ws, **kw)


def _snap(out):
    return [t.clone() for t in (out.g_logp, out.g_value, out.losses)]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_vtrace_kernel_vs_oracle64(cuda, shape, setting):
    kw, use_ent = SETTINGS[setting]
    c = _case(shape)
    T, B = c["lpn"].shape
    ref = vtrace_oracle64(c["lpn"], c["lpo"], c["val"], c["rew"], c["done"],
                          c["ent"] if use_ent else None, **dict(DEFAULTS, **kw))
    ws = VTraceWorkspace()
    out = _run(c, cuda, ws, kw, use_ent)
    d = torch.float64
    vs, adv = out.vs.cpu().to(d), out.adv.cpu().to(d)
    gl, gv, losses = out.g_logp.cpu().to(d), out.g_value.cpu().to(d), out.losses.cpu().to(d)
    print(f"{shape} {setting}: max |err| vs {float((vs - ref['vs']).abs().max()):.3g} "
          f"adv {float((adv - ref['adv']).abs().max()):.3g} "
          f"losses {(losses - ref['losses']).abs().tolist()}")
    assert gl.shape == (T, B) and gv.shape == (T + 1, B)
    torch.testing.assert_close(vs, ref["vs"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(adv, ref["adv"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gl, ref["g_logp"], rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(gv[:T], ref["g_value"], rtol=1e-4, atol=1e-8)
    assert float(gv[T].abs().max()) == 0.0  # (poisoned with NaN before the call)
    torch.testing.assert_close(losses, ref["losses"], rtol=1e-4, atol=1e-5)
    if not use_ent:
        assert float(losses[2]) == 0.0
    assert out.g_ent == -dict(DEFAULTS, **kw)["entropy_cost"] / float(T * B)
    if SHAPES[shape][3]:  # all dones: no recurrence left, in fp64 closed form
        v, r = c["val"].to(d), c["rew"].to(d)
        cl = dict(DEFAULTS, **kw)["reward_clip"]
        r = r.clamp(-cl, cl) if cl > 0 else r
        rho = torch.exp(c["lpn"].to(d) - c["lpo"].to(d)).clamp(max=dict(DEFAULTS, **kw)["rho_bar"])
        torch.testing.assert_close(vs, v[:T] + rho * (r - v[:T]), rtol=1e-4, atol=1e-4)
    # the targets are optional outputs: without them the gradients and losses are the same bits
    snap = _snap(out)
    out2 = _run(c, cuda, ws, kw, use_ent, want_targets=False)
    assert out2.vs is None and out2.adv is None
    for a, b in zip(snap, _snap(out2)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("setting", ["defaults", "nondefault"])
def test_vtrace_kernel_is_bit_reproducible(cuda, setting):
    kw, _ = SETTINGS[setting]
    c = _case("37x300")
    ws = VTraceWorkspace()
    full = lambda o: _snap(o) + [o.vs.clone(), o.adv.clone()]  # noqa: E731
    a = full(_run(c, cuda, ws, kw))
    b = full(_run(c, cuda, ws, kw))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the same workspace at another B (buffers re-sized), then back
    _run(_case("3x16641"), cuda, ws, kw)
    _run(_case("5x63"), cuda, ws, kw)
    for x, y in zip(a, full(_run(c, cuda, ws, kw))):
        assert torch.equal(x, y)
