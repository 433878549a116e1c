"""A decoder whose vocabulary (70,001) no workgroup can hold: device sampling,
serving and served log-probabilities run through the streaming kernels of
csrc/sample_wide.hip; beam search stays refused.  INT8, 2 layers, 2 heads x 64,
synthetic weights."""
import numpy as np
import pytest

from test_decoder_gpu import _int8_model, _make_gpu_decoder
from test_logprob_rows_gpu import ktol

pytestmark = pytest.mark.gpu

V = 70001


@pytest.fixture(scope="module")
def weights(oracle):
    return _int8_model(oracle, L=2, H=2, D=64, V=V, S=64, seed=6)


def test_device_sampling_step(gpu, weights):
    """test_decoder_device_sampling's check at this vocabulary: one step's ids
    against the oracle sampler on the step's own logits (row terms 0 .. 3,
    counter = position 0)."""
    import torch
    from oracle.oracle import sample_rows
    dec = _make_gpu_decoder(weights, max_batch=4)
    dec.set_sampling(0.8, 40, 0.9, 1)
    dec.begin_synthetic(4, 0, 0, False)
    logits = torch.empty((4, V), device="cuda")
    nxt = dec.step([3, 1, 4, 69999], logits_ptr=logits.data_ptr(), want_next=True)
    torch.cuda.synchronize()
    ref, margin, near = sample_rows(logits.cpu().numpy(), 0.8, 40, 0.9, seed=1, counter=0,
                                    neighbours=True)
    for r in range(4):
        assert nxt[r] == ref[r] or (margin[r] < 1e-4 and nxt[r] in near[r]), (r, nxt, ref, margin)


def test_serving(gpu, weights):
    import torch
    dec = _make_gpu_decoder(weights, max_batch=4)
    prompts = [[5, 69000, 17, 2], [40000, 9]]
    greedy = dec.generate(prompts[0], 6, 1.0)
    buf = torch.empty((4, V), device="cuda")
    dec.serve_begin()
    assert dec.submit(prompts[0], 6) == 0
    assert dec.submit(prompts[1], 6, temperature=0.8, top_k=40, top_p=0.9, seed=1, logprobs=3) == 1
    ids, checked = {0: [], 1: []}, 0
    while sum(dec.serve_stats()[k] for k in ("live", "waiting")):
        ev = dec.serve_step(buf.data_ptr())
        lg = buf.cpu().numpy()
        for (rid, tok, idx, row, fin), lp in zip(ev, dec.serve_logprobs()):
            ids[rid].append(tok)
            if rid == 0:
                assert lp is None
                continue
            x = lg[row].astype(np.float64)  # the step's own logits row
            m = x.max()
            lse = np.log(np.exp(x - m).sum() + 1e-6)
            chosen, top = lp
            assert chosen <= 0.0 and abs(chosen - ((x[tok] - m) - lse)) <= ktol((x[tok] - m) - lse)
            assert [t for t, _ in top] == list(np.lexsort((np.arange(V), -x))[:3])
            for t, v in top:
                assert abs(v - ((x[t] - m) - lse)) <= ktol((x[t] - m) - lse), (idx, t, v)
            checked += 1
        assert len(ids[0]) + len(ids[1]) < 50
    dec.serve_end()
    assert checked == 6 and ids[0] == list(greedy)[-6:]
    with pytest.raises(RuntimeError, match="vocab_size > 65536"):
        dec.beam_search(prompts[0], 2, 4)
