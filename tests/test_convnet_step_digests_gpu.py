"""The fused MNIST step's results against digests recorded with the build of the commit
before the step kernels were last changed (tests/helpers/step_digests.py,
tests/golden/convnet_step_digests.json): the pooled tile, the argmax codes, every weight and
the metric sums after steps 1 and 3 are the recorded bits, in both instantiations of the
kernels (specialised and generic), with uint8 and fp32 rows, plain SGD and nesterov."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import step_digests  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("opt", ["sgd", "nesterov"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "fp32"])
def test_step_digests(u8, opt, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    want = step_digests.load_golden()[step_digests.config_id(u8, opt)]
    spec = step_digests.run_arm(monkeypatch.setenv, u8, opt, True)
    gen = step_digests.run_arm(monkeypatch.setenv, u8, opt, False)
    for st in ("step1", "step3"):
        print(st, "specialised", spec[st])
        print(st, "generic    ", gen[st])
    assert spec == gen, "the two instantiations disagree"
    assert set(want) == {"step1", "step3"} and all(len(want[st]) == 9 for st in want), "golden file incomplete"
    for st in want:
        diff = sorted(k for k in want[st] if spec[st].get(k) != want[st][k])
        assert not diff, (st, diff)
