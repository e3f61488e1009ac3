"""runtime/outputs.py on an MI355X: the one device-to-host copy gives the same host bytes on the
current stream (as graph replays need it) and on the D2H stream, for full rows and compact scores,
at a shape that is no multiple of 8 and below a wave (5 rows of 97: the int32 tokens do not start
on a multiple of 4 bytes behind the fp16 rows unless the copy aligns them)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as tr  # noqa: E402

gpu = pytest.mark.gpu
HAVE_GPU = torch.cuda.is_available()
needs_gpu = pytest.mark.skipif(not HAVE_GPU, reason="no GPU")
DEV = torch.device("cuda", 0)
ROWS, V = 5, 97


@gpu
@needs_gpu
@pytest.mark.parametrize("K", [0, 3])
def test_same_stream_and_d2h_stream_copies_agree(tmp_path, K):
    from flexible_llm_sharding_amd.ops import get_ops
    from flexible_llm_sharding_amd.runtime.activations import ActivationStore
    from flexible_llm_sharding_amd.runtime.outputs import CallResults, Outputs
    d2h = torch.cuda.Stream(DEV)
    store = ActivationStore("cpu", DEV, str(tmp_path), d2h_stream=d2h)
    try:
        out = Outputs("next_token", K, None, None, get_ops(DEV), DEV, lambda: store, d2h)
        probs = torch.rand(ROWS, V, generator=torch.Generator().manual_seed(5)).half().to(DEV)
        f = probs.cpu().numpy()
        am = f.astype(np.float32).argmax(-1)           # (numpy: the first index of the maximum)
        batch = SimpleNamespace(prompt_ids=[1, 0], n_suffix=[2, 3], draft=None)
        same = out.start(batch, probs, 0, None)
        other = out.start(batch, probs, 0, d2h)
        assert same.event is None and other.event is not None
        assert same.pool_buf.data_ptr() != other.pool_buf.data_ptr()
        torch.cuda.current_stream(DEV).synchronize()
        other.event.synchronize()
        a, b = [h.numpy().copy() for h in same.host], [h.numpy().copy() for h in other.host]
        assert len(a) == len(b) == (4 if K else 2)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        if K:
            ids, vals = tr.ref_topk(f, K)
            assert np.array_equal(a[0], ids) and np.array_equal(a[1], am)
            assert np.array_equal(a[2].view(np.uint16), vals)
            assert np.array_equal(a[3].view(np.uint16), tr.ref_picked(f, am))
        else:
            assert a[0].dtype == np.float16 and np.array_equal(a[0].view(np.uint16), f.view(np.uint16))
            assert a[1].dtype == np.int32 and np.array_equal(a[1], am)
        got = [CallResults.begin([None, None]), CallResults.begin([None, None])]
        out.collect([same], got[0])
        out.collect([other], got[1])
        assert got[0].d2h_bytes == got[1].d2h_bytes == (ROWS * (6 * K + 6) if K else ROWS * (2 * V + 4))
        r = 0
        for pid, ns in zip(batch.prompt_ids, batch.n_suffix):
            for res in got:
                o = res.outputs[pid]
                assert o.shape == (ns, 1, K or V)
                if K:
                    assert np.array_equal(o["id"][:, 0], a[0][r:r + ns]) and np.array_equal(o["p"][:, 0], a[2][r:r + ns])
                    assert np.array_equal(res.token_probs[pid][:, 0], a[3][r:r + ns])
                else:
                    assert np.array_equal(o[:, 0].view(np.uint16), f[r:r + ns].view(np.uint16))
                    assert res.token_probs[pid] is None
                assert res.tokens[pid].dtype == np.int64 and np.array_equal(res.tokens[pid][:, 0], am[r:r + ns])
            r += ns
    finally:
        store.close()
