"""Host logic for 128-channel attention heads (no GPU): the UNet constructs them -- SpatialTransformer included -- and the execution plan
routes a 128-wide layer exactly as it routes the 64-wide form of the same layer (plans built on CPU tensors, as in test_plan_cpu.py:
construction only queries the C-ABI's host-side size functions)."""
import pytest
import torch

from bbdm_amd import _lib, unet

TINY = dict(image_size=32, in_channels=3, model_channels=256, out_channels=3, num_res_blocks=1, attention_resolutions=(1,),
            channel_mult=(1,), use_scale_shift_norm=True, resblock_updown=True, condition_key="nocond")


def _attn_ops(ops):
    return [(str(getattr(n, "entry", n)), str(n)) for n, _ in ops if "attention" in str(n) or "affine_bound" in str(n)]


def test_spatial_transformer_takes_128_wide_heads():
    """openaimodel.py:546-565: num_head_channels = 128, or num_heads = 4 at 512 channels -> d_head 128; other widths still raise."""
    m = unet.UNetModel(**dict(TINY, image_size=8, model_channels=128, channel_mult=(1, 2), use_spatial_transformer=True,
                              context_dim=3, condition_key="SpatialRescaler", num_head_channels=128))
    sts = [mod for mod in m.modules() if isinstance(mod, unet.SpatialTransformer)]
    assert sts and {(st.n_heads, st.d_head) for st in sts} == {(1, 128), (2, 128)}
    m = unet.UNetModel(**dict(TINY, image_size=8, model_channels=512, use_spatial_transformer=True, context_dim=3,
                              condition_key="SpatialRescaler", num_heads=4, num_head_channels=-1))
    assert {(st.n_heads, st.d_head) for st in m.modules() if isinstance(st, unet.SpatialTransformer)} == {(4, 128)}
    with pytest.raises(NotImplementedError, match="head width 256"):
        unet.UNetModel(**dict(TINY, image_size=8, use_spatial_transformer=True, context_dim=3, condition_key="SpatialRescaler",
                              num_head_channels=256))


def test_attention_block_128_wide_heads_construct():
    m = unet.UNetModel(**dict(TINY, num_head_channels=128))
    assert {ab.num_heads for ab in m.modules() if isinstance(ab, unet.AttentionBlock)} == {2}


def test_long_sequence_128_wide_plan_takes_the_presplit_route():
    """An AttentionBlock of 2 x 128 channels at T = 1024 (32 x 32) is planned like its 4 x 64 form: the K / V planes + planes launches
    (on the fp16-pair planes under the projection's bound by default), the planes in the Winograd scratch, sized for the layer."""
    lib = _lib.load()
    x = torch.zeros(2, 3, 32, 32)
    got = {}
    for hc in (64, 128):
        m = unet.UNetModel(**dict(TINY, num_head_channels=hc)).eval()
        plan = m._plan_for(x, False)
        got[hc] = (_attn_ops(plan.ops), plan)
    ops64, ops128 = got[64][0], got[128][0]
    assert ops128 == ops64
    entries = [e for e, _ in ops128]
    assert "bbdm_attention_kv_planes_h2_f32" in entries and "bbdm_attention_planes_h2_f32" in entries
    need = lib.bbdm_attention_kv_planes_h2_bytes(2, 1024, 2, 128)
    assert need == lib.bbdm_attention_kv_planes_h2_bytes(2, 1024, 4, 64) > 0
    assert got[128][1]._wino_v_need * 4 >= need
    # the plan's attention launches carry the 128-wide geometry
    heads_ch = {(args[7], args[8]) for n, args in got[128][1].ops if str(getattr(n, "entry", n)) == "bbdm_attention_planes_h2_f32"}
    assert heads_ch == {(2, 128)}
    # ... and the bf16x3 pair where the fp16-pair planes are switched off
    m = unet.UNetModel(**dict(TINY, num_head_channels=128)).eval()
    m.attn_h2 = False
    entries = [e for e, _ in _attn_ops(m._plan_for(x, False).ops) if "attention" in e]
    assert len(entries) >= 6 and entries == ["bbdm_attention_kv_planes_f32", "bbdm_attention_planes_f32"] * (len(entries) // 2)
    assert lib.bbdm_attention_kv_planes_bytes(2, 1024, 2, 128) == lib.bbdm_attention_kv_planes_bytes(2, 1024, 4, 64) > 0


def test_training_plan_sizes_lse_per_128_wide_head():
    """The training plan keeps one log-sum-exp per (image, head, query) for the backward and runs the packed-qkv backward at width 128."""
    m = unet.UNetModel(**dict(TINY, image_size=16, num_head_channels=128)).train()
    plan = m._plan_for(torch.zeros(2, 3, 16, 16), True)
    fw = [args for n, args in plan.ops if str(getattr(n, "entry", n)) == "bbdm_attention_f32"]
    assert len(fw) >= 3 and all(tuple(a[7:9]) == (2, 128) and a[4].t.numel() == 2 * 2 * 256 for a in fw)
    bw = [args for n, args in plan.bops if str(getattr(n, "entry", n)) == "bbdm_attention_bwd_f32"]
    assert len(bw) == len(fw) and all(tuple(a[12:14]) == (2, 128) for a in bw)
