"""F(6x6, 3x3) on an input that is a channel slice of a wider tensor (Plan._conv's in_ld: decoder.convFM.q reads the value half of the
[n, HW, 640] key / value slab): the layer's result, and where the plans use it."""
import pytest
import torch

from golden_util import state_dict

pytestmark = pytest.mark.gpu


def test_f6_layer_on_a_channel_slice_equals_the_contiguous_copy(gpu):
    """Columns 128..639 of a [2, 6, 12, 640] tensor against a contiguous copy of them: the same kernels read the same values, so the
    outputs are bit-equal (ReLU on the input, scale, shift, ReLU on the output included)."""
    from vfloodnet_amd import ops
    g = torch.Generator().manual_seed(640)
    wide = torch.randn(2, 6, 12, 640, generator=g).to(gpu)
    w = torch.randn(256, 512, 3, 3, generator=g) / (512 * 9) ** 0.5
    kw = dict(scale=(1 + 0.1 * torch.randn(256, generator=g)).to(gpu), shift=(0.1 * torch.randn(256, generator=g)).to(gpu),
              relu_in=True, relu_out=True, cfg=ops.wino_gemm_cfg(3, 512), tile=6)
    part = wide[..., 128:]
    assert part.stride(2) == 640 and not part.is_contiguous()
    y_slice = ops.conv2d_winograd(part, w, **kw)
    y_copy = ops.conv2d_winograd(part.contiguous(), w, **kw)
    assert bool(torch.isfinite(y_copy).all()) and float(y_copy.abs().max()) > 0
    assert torch.equal(y_slice, y_copy)


@pytest.mark.parametrize('switch', ['1', '0'])
def test_convFM_q_launches_follow_the_switch(gpu, switch, monkeypatch):
    """The 96x160 plan with F(6x6) on every layer that may take it: decoder.convFM.q is the three Winograd launches (the input transform
    at pixel stride 640) with VFN_WINO_STRIDED_IN on, the one direct launch with it off."""
    from vfloodnet_amd import AFB_URR, engine as E, ops
    monkeypatch.setattr(E, '_WINOGRAD', '2')
    monkeypatch.setattr(E, '_WINOGRAD_F6', '2')
    monkeypatch.setattr(E, '_WINO_STRIDED_IN', switch)
    model = AFB_URR(gpu, update_bank=True).to(gpu).eval()
    model.load_state_dict(state_dict(), strict=True)
    plan = model.engine().plan(96, 160, 2)
    runs, cur = [], None                                   # the launches of the layer, list by list, in order
    for lst in plan.all_lists():
        for l in lst:
            if (l.name or '').startswith('decoder.convFM.q'):
                if cur is None:
                    cur = []
                    runs.append(cur)
                cur.append(l)
            else:
                cur = None
    assert runs
    for run in runs:
        if switch == '1':
            assert [l.fn for l in run] == [ops.winograd_input, ops.conv2d_launch, ops.winograd_output], [l.name for l in run]
            assert run[0].args[-1] == 6 and run[0].args[8] == 640 and run[0].args[7] == 512      # tile, ld_x, channels
        else:
            assert [l.fn for l in run] == [ops.conv2d_launch] and run[0].args[0].in_ld == 640, [l.name for l in run]
