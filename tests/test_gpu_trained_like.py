"""Per-launch parity (tests/test_gpu_launch_parity.py: untouched-or-fully-written blocks, every op evaluated from the device's own inputs
against op_ref's bound E, carry-over to the default plan) on the trained-like weights of tests/trained_like.py: negative gamma, dead
channels, per-channel gains spread over 2^6.5, activations in the hundreds and thousands, SE gates pinned at 0 and 1, folded weights in the
fp16 subnormal range and, under "hot_heads", logits and box regressions far outside what the synthetic heads give. The bound is op_ref's one
rule, as it stands. tests/test_lowering_trained_like.py holds, on the CPU, that the regimes reach those ranges on the reference alone."""
import numpy as np
import pytest
import torch

import test_gpu_launch_parity as lp
import trained_like
from demonet_amd import models, synth

pytestmark = pytest.mark.gpu

V3, V2 = lp.V3, lp.V2
# (configuration of test_gpu_launch_parity.py: model, classes, n, knobs, size), regime
CONFIGS = [((V3, 91, 2, {}, None), "spread"),
           ((V2, 21, 3, {}, 160), "spread"),
           ((V2, 21, 2, {}, 320), "spread"),
           (("ssd300_vgg16", 91, 2, {}, None), "spread"),
           ((V3, 91, 2, {}, None), "hot_heads"),
           ((V3, 91, 2, {"DN_EXPDW": "0"}, None), "spread")]      # the unfused blocks: held bit-identical to the fused ones on synthetic values only


def _tid(c):
    return lp._cid(c[0]) + "-" + c[1]


@pytest.mark.parametrize("cfg,regime", CONFIGS, ids=[_tid(c) for c in CONFIGS])
def test_launch_parity_on_trained_like_weights(cfg, regime):
    res = lp._run(cfg, regime)
    print("\n" + lp._report(res, _tid((cfg, regime))))
    st = res["stats"]
    if st.worst:
        lab = max(st.worst, key=st.worst.get)
        print(f"  closest to the bound: {st.worst[lab]:.6f}  {st.where[lab]}")
    assert not res["fails"], "\n".join(res["fails"][:20])
    assert sum(st.count.values()) > 0 and all(np.isfinite(v) for v in st.worst.values())


def test_a_checkpoint_the_lowering_refuses_raises_before_any_launch():
    """The guard of demonet_amd/plan.py surfaces through SSD._plan: load_state_dict takes the checkpoint as it is, model(images) raises the
    ValueError that names the key, no plan exists afterwards, and the model runs again once good weights are loaded."""
    m = trained_like.load(models.ssd_lite_mobilenet_v2(num_classes=21, image_size=160, score_thresh=0.01), "spread")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["backbone.body.3.conv.0.0.weight"][5, 3, 0, 0] = float("nan")
    sd["backbone.body.3.conv.0.1.running_var"][7] = 0.0
    sd["backbone.body.3.conv.0.1.weight"][7] = 3000.0
    assert not m.load_state_dict(sd).missing_keys
    m = m.cuda()
    img = torch.from_numpy(synth.images(11, 1, 160, 160)[0]).cuda()
    with pytest.raises(ValueError, match="non-finite parameter: state_dict\\['backbone.body.3.conv.0.0.weight'\\] is nan at output channel 5 "):
        m([img])
    assert m._handle is None
    sd["backbone.body.3.conv.0.0.weight"][5, 3, 0, 0] = 0.25
    sd["backbone.body.3.conv.0.0.weight"][7] = 0.5               # 0.5 * 3000 / sqrt(0 + 1e-5) = 4.7e5: past fp16
    m.load_state_dict(sd)
    with pytest.raises(ValueError, match="folded value out of range: .*'backbone.body.3.conv.0.1' of state_dict\\['backbone.body.3.conv.0.0.weight'\\] "
                                         "is .* at output channel 7 "):
        m([img])
    assert m._handle is None
    trained_like.load(m, "spread")
    out = m([img])[0]
    assert torch.isfinite(out["boxes"]).all() and torch.isfinite(out["scores"]).all() and out["scores"].numel() > 0
