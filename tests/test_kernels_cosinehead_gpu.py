"""``fd_cosine_logits_fwd`` / ``fd_cosine_logits_bwd`` (the zero-shot classifier head) directly against fp64 on the fp16 library (GPU): the table, the
gates and the layout of tests/cosinehead_cases.py -- odd-offset views with sentinel guards, strided embedding rows, the all-zero row, the row that
equals a class direction --, equal bits call after call and on a side stream, and the host refusals, which launch nothing."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cosinehead_cases as C  # noqa: E402
from finetune_fair_diffusion_amd import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cosine_head_table_against_fp64(dev):
    C.run_table(ops, dev, "fp16 library")


def test_cosine_head_calls_give_equal_bits_also_on_a_side_stream(dev):
    C.repeat_bits(ops, dev)


def test_cosine_head_refusals_launch_nothing(dev):
    """K = 17, E = 0, lde < E and a null buffer: FD_ERR_ARG, ``fd_last_error`` names the entry point, and no output element changes."""
    L = lib.get()
    N, E, K = 3, 48, 2
    p = C.Problem(dev, (N, E, K, 0))
    v = {n: p.buf.view(n) for n in ("e", "t_hat", "logits", "inv_norm", "d_logits", "d_e", "lg_in", "inv_in")}
    before = p.buf.flat.clone()
    ptr = lambda n: ctypes.c_void_p(v[n].data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(e="e", lde=E, t="t_hat", lg="logits", inv="inv_norm", n=N, ee=E, k=K):
        return L.fd_cosine_logits_fwd(ptr(e) if e else None, lde, ptr(t) if t else None, 100.0, ptr(lg) if lg else None, ptr(inv) if inv else None, n, ee, k, stream)

    def bwd(lde=E, dl="d_logits", de="d_e", n=N, ee=E, k=K):
        return L.fd_cosine_logits_bwd(ptr("e"), lde, ptr("t_hat"), ptr("lg_in"), ptr("inv_in"), ptr(dl) if dl else None, 100.0, ptr(de) if de else None, n, ee, k, stream)

    refused = [("fd_cosine_logits_fwd", lambda: fwd(k=17)), ("fd_cosine_logits_fwd", lambda: fwd(ee=0)), ("fd_cosine_logits_fwd", lambda: fwd(lde=E - 1)),
               ("fd_cosine_logits_fwd", lambda: fwd(inv=None)), ("fd_cosine_logits_fwd", lambda: fwd(e=None)), ("fd_cosine_logits_fwd", lambda: fwd(n=0)),
               ("fd_cosine_logits_bwd", lambda: bwd(k=17)), ("fd_cosine_logits_bwd", lambda: bwd(ee=0)), ("fd_cosine_logits_bwd", lambda: bwd(lde=E - 1)),
               ("fd_cosine_logits_bwd", lambda: bwd(de=None)), ("fd_cosine_logits_bwd", lambda: bwd(dl=None)), ("fd_cosine_logits_bwd", lambda: bwd(k=0))]
    for name, call in refused:
        rc = call()
        msg = L.fd_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":"), (name, rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(p.buf.flat, before), "a refused call wrote to a buffer"
    with pytest.raises(RuntimeError, match="fd_cosine_logits_fwd"):       # the wrapper turns the code into an exception that carries the message
        ops.cosine_logits(torch.zeros(2, 8, device=dev), torch.zeros(17, 8, device=dev), 1.0)
    assert fwd() == 0 and bwd() == 0                                        # the same calls with nothing wrong are accepted
    torch.cuda.synchronize()
