"""Images per workgroup round of the conv-trunk kernels, as the kernel library chooses them
(conv.hip / resblock.hip, the mbk_*_imgs exports: pure arithmetic, no GPU).

The table below was recorded from the Python sizing rules these exports replaced (the encoder's
former ``_imgs_fwd`` / ``_imgs_wgrad`` and its inline residual-block formulas), for every layer of
the (16, 32, 32) trunk on 8, 10, 16 and 24 maps, the 4-stage 24x24 trunk and GridNet's one-layer
``channels=(32,)`` encoder. A round size decides the summation order of a weight gradient's
partial rows and the measured speed, so a kernel-layout edit that moves one has to show up here."""
import pytest

from microbeast_amd import _native as N
from microbeast_amd.ops.encoder import HipEncoder

CONFIGS = {
    "impala8": (8, (16, 32, 32)), "impala10": (10, (16, 32, 32)), "impala16": (16, (16, 32, 32)),
    "impala24": (24, (16, 32, 32)), "deep24": (24, (16, 32, 32, 32)),
    # GridNet uses layer 0 of a one-stage 32-channel encoder only (ops/pixconv.py)
    "gridnet8": (8, (32,)), "gridnet10": (10, (32,)), "gridnet16": (16, (32,)),
    "gridnet24": (24, (32,)),
}

# (config, layer): (cin, cout, H, W, bits, pool, fwd, fp8, dgrad, wgrad, unpool1, unpool2,
#                   res_bwd16, res_blk32, res_bwd32); None: the rule does not apply
TABLE = {
    ("impala8", 0): (32, 16, 8, 8, 1, 1, 4, 4, None, 4, 1, 2, None, None, None),
    ("impala8", 1): (16, 16, 4, 4, 0, 0, 16, 32, 16, 32, None, None, 8, None, None),
    ("impala8", 2): (16, 16, 4, 4, 0, 0, 16, 32, 16, 32, None, None, 8, None, None),
    ("impala8", 3): (16, 16, 4, 4, 0, 0, 16, 32, 16, 32, None, None, 8, None, None),
    ("impala8", 4): (16, 16, 4, 4, 0, 0, 16, 32, 16, 32, None, None, 8, None, None),
    ("impala8", 5): (16, 32, 4, 4, 0, 1, 16, 16, 16, 16, None, None, None, None, None),
    ("impala8", 6): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala8", 7): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala8", 8): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala8", 9): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala8", 10): (32, 32, 2, 2, 0, 1, 16, 32, 32, 32, None, None, None, None, None),
    ("impala8", 11): (32, 32, 1, 1, 0, 0, 64, 128, 64, 64, None, None, None, 16, 53),
    ("impala8", 12): (32, 32, 1, 1, 0, 0, 64, 128, 64, 64, None, None, None, 16, 53),
    ("impala8", 13): (32, 32, 1, 1, 0, 0, 64, 128, 64, 64, None, None, None, 16, 53),
    ("impala8", 14): (32, 32, 1, 1, 0, 0, 64, 128, 64, 64, None, None, None, 16, 53),
    ("impala10", 0): (32, 16, 10, 10, 1, 1, 2, 5, None, 5, 1, 2, None, None, None),
    ("impala10", 1): (16, 16, 5, 5, 0, 0, 20, 20, 20, 20, None, None, 8, None, None),
    ("impala10", 2): (16, 16, 5, 5, 0, 0, 20, 20, 20, 20, None, None, 8, None, None),
    ("impala10", 3): (16, 16, 5, 5, 0, 0, 20, 20, 20, 20, None, None, 8, None, None),
    ("impala10", 4): (16, 16, 5, 5, 0, 0, 20, 20, 20, 20, None, None, 8, None, None),
    ("impala10", 5): (16, 32, 5, 5, 0, 1, 10, 10, 10, 10, None, None, None, None, None),
    ("impala10", 6): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("impala10", 7): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("impala10", 8): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("impala10", 9): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("impala10", 10): (32, 32, 3, 3, 0, 1, 14, 28, 14, 28, None, None, None, None, None),
    ("impala10", 11): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala10", 12): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala10", 13): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala10", 14): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala16", 0): (32, 16, 16, 16, 1, 1, 1, 2, None, 2, 1, 2, None, None, None),
    ("impala16", 1): (16, 16, 8, 8, 0, 0, 8, 8, 8, 8, None, None, 4, None, None),
    ("impala16", 2): (16, 16, 8, 8, 0, 0, 8, 8, 8, 8, None, None, 4, None, None),
    ("impala16", 3): (16, 16, 8, 8, 0, 0, 8, 8, 8, 8, None, None, 4, None, None),
    ("impala16", 4): (16, 16, 8, 8, 0, 0, 8, 8, 8, 8, None, None, 4, None, None),
    ("impala16", 5): (16, 32, 8, 8, 0, 1, 4, 4, 4, 4, None, None, None, None, None),
    ("impala16", 6): (32, 32, 4, 4, 0, 0, 16, 32, 16, 16, None, None, None, 14, 8),
    ("impala16", 7): (32, 32, 4, 4, 0, 0, 16, 32, 16, 16, None, None, None, 14, 8),
    ("impala16", 8): (32, 32, 4, 4, 0, 0, 16, 32, 16, 16, None, None, None, 14, 8),
    ("impala16", 9): (32, 32, 4, 4, 0, 0, 16, 32, 16, 16, None, None, None, 14, 8),
    ("impala16", 10): (32, 32, 4, 4, 0, 1, 8, 16, 16, 16, None, None, None, None, None),
    ("impala16", 11): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala16", 12): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala16", 13): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala16", 14): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("impala24", 0): (32, 16, 24, 24, 1, 1, 1, 1, None, 1, 1, 1, None, None, None),
    ("impala24", 1): (16, 16, 12, 12, 0, 0, 3, 3, 3, 3, None, None, 2, None, None),
    ("impala24", 2): (16, 16, 12, 12, 0, 0, 3, 3, 3, 3, None, None, 2, None, None),
    ("impala24", 3): (16, 16, 12, 12, 0, 0, 3, 3, 3, 3, None, None, 2, None, None),
    ("impala24", 4): (16, 16, 12, 12, 0, 0, 3, 3, 3, 3, None, None, 2, None, None),
    ("impala24", 5): (16, 32, 12, 12, 0, 1, 1, 3, 3, 1, None, None, None, None, None),
    ("impala24", 6): (32, 32, 6, 6, 0, 0, 7, 14, 7, 7, None, None, None, 8, 4),
    ("impala24", 7): (32, 32, 6, 6, 0, 0, 7, 14, 7, 7, None, None, None, 8, 4),
    ("impala24", 8): (32, 32, 6, 6, 0, 0, 7, 14, 7, 7, None, None, None, 8, 4),
    ("impala24", 9): (32, 32, 6, 6, 0, 0, 7, 14, 7, 7, None, None, None, 8, 4),
    ("impala24", 10): (32, 32, 6, 6, 0, 1, 3, 7, 7, 7, None, None, None, None, None),
    ("impala24", 11): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("impala24", 12): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("impala24", 13): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("impala24", 14): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("deep24", 0): (32, 16, 24, 24, 1, 1, 1, 1, None, 1, 1, 1, None, None, None),
    ("deep24", 1): (16, 16, 12, 12, 0, 0, 3, 3, 3, 3, None, None, 2, None, None),
    ("deep24", 2): (16, 16, 12, 12, 0, 0, 3, 3, 3, 3, None, None, 2, None, None),
    ("deep24", 3): (16, 16, 12, 12, 0, 0, 3, 3, 3, 3, None, None, 2, None, None),
    ("deep24", 4): (16, 16, 12, 12, 0, 0, 3, 3, 3, 3, None, None, 2, None, None),
    ("deep24", 5): (16, 32, 12, 12, 0, 1, 1, 3, 3, 1, None, None, None, None, None),
    ("deep24", 6): (32, 32, 6, 6, 0, 0, 7, 14, 7, 7, None, None, None, 8, 4),
    ("deep24", 7): (32, 32, 6, 6, 0, 0, 7, 14, 7, 7, None, None, None, 8, 4),
    ("deep24", 8): (32, 32, 6, 6, 0, 0, 7, 14, 7, 7, None, None, None, 8, 4),
    ("deep24", 9): (32, 32, 6, 6, 0, 0, 7, 14, 7, 7, None, None, None, 8, 4),
    ("deep24", 10): (32, 32, 6, 6, 0, 1, 3, 7, 7, 7, None, None, None, None, None),
    ("deep24", 11): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("deep24", 12): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("deep24", 13): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("deep24", 14): (32, 32, 3, 3, 0, 0, 14, 28, 14, 28, None, None, None, 16, 12),
    ("deep24", 15): (32, 32, 3, 3, 0, 1, 14, 28, 14, 28, None, None, None, None, None),
    ("deep24", 16): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("deep24", 17): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("deep24", 18): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("deep24", 19): (32, 32, 2, 2, 0, 0, 32, 64, 32, 32, None, None, None, 16, 29),
    ("gridnet8", 0): (32, 32, 8, 8, 1, 1, 2, 4, None, 4, 1, 2, None, None, None),
    ("gridnet10", 0): (32, 32, 10, 10, 1, 1, 2, 2, None, 2, 1, 2, None, None, None),
    ("gridnet16", 0): (32, 32, 16, 16, 1, 1, 1, 1, None, 1, 1, 1, None, None, None),
    ("gridnet24", 0): (32, 32, 24, 24, 1, 1, 1, 1, None, 1, 1, 1, None, None, None),
}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_round_sizes_match_the_recorded_table(config):
    k = N.kernels()
    size, channels = CONFIGS[config]
    layers = HipEncoder(size, size, 27, channels).layers
    if config.startswith("gridnet"):
        layers = layers[:1]
    assert sorted(i for c, i in TABLE if c == config) == list(range(len(layers)))
    for i, L in enumerate(layers):
        (cin, cout, H, W, bits, pool, fwd, fp8, dgrad, wgrad, unpool1, unpool2, res_bwd16,
         res_blk32, res_bwd32) = TABLE[config, i]
        assert (L.cin, L.cout, L.H, L.W, int(L.bits), int(L.pool)) == (cin, cout, H, W, bits, pool)
        what = f"{config} layer {i}"
        assert k.mbk_conv_fwd_imgs(bits, cin, cout, H, W, pool, 0) == fwd, what
        assert k.mbk_conv_fwd_imgs(bits, cin, cout, H, W, pool, 1) == fp8, what
        if dgrad is not None:  # the forward of (cout, cin) at the layer's input size
            assert k.mbk_conv_fwd_imgs(0, cout, cin, H, W, 0, 0) == dgrad, what
        assert k.mbk_conv_wgrad_imgs(bits, cin, cout, H, W, 0) == wgrad, what
        if unpool1 is not None:
            assert k.mbk_conv_wgrad_imgs(bits, cin, cout, H, W, 1) == unpool1, what
            assert k.mbk_conv_wgrad_imgs(bits, cin, cout, H, W, 2) == unpool2, what
        if res_bwd16 is not None:
            assert k.mbk_res_bwd16_imgs(H, W) == res_bwd16, what
        if res_blk32 is not None:
            assert k.mbk_res_blk32_fwd_imgs(H, W) == res_blk32, what
            assert k.mbk_res_bwd32_imgs(H, W) == res_bwd32, what


def test_stage_fusion_fits_where_it_runs():
    """The stage-0 residual kernel also runs stage 1's conv on these maps (8, 10, 16, 24 trunks)."""
    for s in (4, 5, 8, 12):
        assert N.kernels().mbk_res_fwd16_stage_ok(s, s) == 1


def test_no_such_map_is_zero():
    k = N.kernels()
    assert k.mbk_conv_fwd_imgs(0, 16, 16, 0, 8, 0, 0) == 0
    assert k.mbk_conv_wgrad_imgs(0, 16, 16, 8, 0, 0) == 0
    assert k.mbk_res_bwd16_imgs(0, 0) == 0 and k.mbk_res_bwd32_imgs(0, 4) == 0
    assert k.mbk_res_blk32_fwd_imgs(4, 0) == 0 and k.mbk_res_fwd16_stage_ok(0, 0) == 0
