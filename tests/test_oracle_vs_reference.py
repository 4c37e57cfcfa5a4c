"""CPU: restatement vs the reference, through what the reference itself computed (tests/golden/g12_vs_reference.npz, written by
tests/golden/make_golden.py from the reference's FootprintNetwork / LossManager).

Outputs are held to 1e-5 of each tensor's max: generated and checked on the same kind of host they agree bit for bit (the restatement
runs the reference's own op sequence), and the margin only admits the rounding of another CPU's kernels."""
import torch

from oracle import restatement as R
from tests.golden.digest import compare, load, sparse_sample


def test_state_dict_layout_matches_reference():
    gold = load("g12_vs_reference")
    spec = R.state_spec()
    assert [str(k) for k in gold["layout.keys"]] == [s[0] for s in spec]
    assert [tuple(int(d) for d in row if d >= 0) for row in gold["layout.shapes"]] == [tuple(s[1]) for s in spec]


def test_forward_backward_and_loss_match_reference():
    gold = load("g12_vs_reference")
    P, B = R.make_state(tag="vsref")
    batch = R.make_batch(2, 64, 64, tag="vsref")
    tr = R.OracleTrainer(P, B)
    out, l = tr.forward_backward(batch)
    assert sorted("out" + k for k in out) == sorted(f for f in gold.files if f.startswith("out"))
    for k in out:
        compare(gold, "out" + k, out[k], rtol=1e-5)
    ours = {repr(k): float(v) for k, v in l.items()}
    for k, v in zip(gold["loss.keys"], gold["loss.values"]):
        assert abs(ours[str(k)] - float(v)) <= 2e-6 * max(1.0, abs(float(v))), k
    names = [str(k) for k in gold["grad.names"]]
    assert set(names) == set(tr.P)
    off = gold["grad.sample_offsets"]
    for i, k in enumerate(names):
        p = tr.P[k]
        if gold["grad.none"][i]:
            assert p.grad is None, k
            continue
        scale = float(gold["grad.max"][i]) + 1e-30
        ref = torch.from_numpy(gold["grad.sample"][off[i]:off[i + 1]])
        assert (sparse_sample(p.grad).double() - ref.double()).abs().max().item() / scale < 1e-4, k
        assert abs(p.grad.abs().max().item() - scale) / scale < 1e-4, k
        assert abs(p.grad.double().sum().item() - float(gold["grad.sum"][i])) <= 1e-4 * float(gold["grad.abs"][i]) + 1e-30, k

