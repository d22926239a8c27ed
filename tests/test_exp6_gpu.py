"""exp-6 (race debiasing) on the MI355X: the device expected-transport targets (``fd_ot_expected_targets``) against the host statement,
the tiny-model exp-6 step against the oracle, and the driver end to end."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_models as U  # noqa: E402

pytestmark = pytest.mark.gpu

RACE = [("race", 2, 4)]


@pytest.fixture(scope="module")
def ops():
    from finetune_fair_diffusion_amd import ops as o
    return o


def _probs(N, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(N, 4, generator=g) * scale, dim=-1)


def _device_targets(ops, dev, probs, table):
    from finetune_fair_diffusion_amd.fairness import _corner_cost
    M = _corner_cost([probs.float().numpy()], [4])
    counts, weights = table
    t, u, seats = ops.ot_expected_targets(torch.from_numpy(M).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(weights).to(dev),
                                          return_seats=True)
    torch.cuda.synchronize()
    return M, t.cpu(), u.cpu(), seats.cpu().numpy()


def _check_seats(M, counts, seats):
    """Every composition's seats respect its counts and reach scipy's optimal cost (1e-12 relative)."""
    from scipy.optimize import linear_sum_assignment
    N, K = M.shape
    assert seats.shape == (len(counts), N) and seats.min() >= 0 and seats.max() < K
    for s in range(len(counts)):
        assert (np.bincount(seats[s], minlength=K) == counts[s]).all(), f"composition {s}: counts violated"
        cols = np.repeat(np.arange(K), counts[s])
        r, c = linear_sum_assignment(M[:, cols])
        opt = M[r, cols[c]].sum()
        got = M[np.arange(N), seats[s]].sum()
        assert abs(got - opt) <= 1e-12 * max(1.0, abs(opt)), f"composition {s}: cost {got} vs optimal {opt}"


@pytest.mark.parametrize("N", [1, 5, 32, 64, 128])
def test_expected_targets_kernel_matches_host(ops, dev, N):
    """fd_ot_expected_targets against the host statement (scipy per composition, sequential fp64 sum) on generic probabilities with the
    product's own table: targets equal, uncertainties bit-equal in fp64; every composition's seats are an optimal assignment."""
    from finetune_fair_diffusion_amd.fairness import composition_table, expected_transport_targets
    probs = _probs(N, 70 + N)
    table = composition_table(N)
    M, t, u, seats = _device_targets(ops, dev, probs, table)
    th, uh = expected_transport_targets(probs)
    assert t.dtype == torch.int32 and u.dtype == torch.float64
    assert t.long().tolist() == th.tolist()
    assert u.numpy().tobytes() == uh.numpy().tobytes(), float((u - uh).abs().max())
    _check_seats(M, table[0], seats)
    # the same through the public entry (device=), with rows that carry no face
    pr = torch.cat([probs[: N // 2], torch.full((3, 4), -1.0), probs[N // 2:]])
    td, ud = expected_transport_targets(pr, device=dev)
    tr, ur = expected_transport_targets(pr)
    assert td.tolist() == tr.tolist() and ud.numpy().tobytes() == ur.numpy().tobytes()
    print(f"N={N}: {len(table[0])} compositions, targets {np.bincount(th.numpy(), minlength=4).tolist()}, max uncertainty {float(uh.max()):.4f}")


@pytest.mark.parametrize("N", [8, 32])
def test_expected_targets_kernel_degenerate_inputs(ops, dev, N):
    """Duplicate rows and saturated one-hot rows (many optimal plans): every composition is still seated feasibly at optimal cost, and two
    runs give identical outputs."""
    from finetune_fair_diffusion_amd.fairness import composition_table
    base = _probs(4, 900 + N)
    rows = [base[i % 4] for i in range(N // 2)]
    rows += [F.one_hot(torch.tensor(i % 4), 4).float() for i in range(N - N // 2)]
    probs = torch.stack(rows)
    table = composition_table(N)
    M, t1, u1, s1 = _device_targets(ops, dev, probs, table)
    _check_seats(M, table[0], s1)
    _, t2, u2, s2 = _device_targets(ops, dev, probs, table)
    assert torch.equal(t1, t2) and u1.numpy().tobytes() == u2.numpy().tobytes() and (s1 == s2).all()
    assert ((t1 >= 0) & (t1 < 4)).all() and bool(torch.isfinite(u1).all()) and float(u1.min()) >= 0.0


def test_expected_targets_rejects_bad_arguments(ops, dev):
    from finetune_fair_diffusion_amd.fairness import composition_table
    counts, weights = composition_table(4)
    M = torch.rand(4, 4, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError):
        ops.ot_expected_targets(M, torch.from_numpy(counts).to(dev)[:0], torch.from_numpy(weights).to(dev)[:0])    # S = 0


def _oracle_race_targets(om, tokens, noises, S, thr, size_face=64):
    """The oracle's own R1 -> classifier race probabilities; the targets from the product's host statement (the expected transport plan),
    thresholded like the step (uncertainty in fp32)."""
    from oracle import fair_step as fs
    from finetune_fair_diffusion_amd.fairness import expected_transport_targets
    with torch.no_grad():
        img = fs.generate_image_no_gradient(tokens, noises, S, om["text_encoder"], om["unet"], om["vae"], om["scheduler"])
        ind, _, chips = fs.SyntheticFaceProvider(size_face)(img)
        lo = om["classifier"](chips[ind])
    p = torch.ones(noises.shape[0], 4) * (-1)
    p[ind] = torch.softmax(lo[:, 2:6], dim=-1)
    t, u = expected_transport_targets(p)
    t = t.clone()
    t[u.float() > thr] = -1
    return t, u, img, p


def test_full_step_exp6_with_oracle_targets(dev):
    """exp-6 at test size (6-logit GenderRace4 head, race columns 2:6, LoRA on the U-Net): the product's step derives the same targets from its
    own R1 through the device solver on the worker thread; the CE loss and the U-Net LoRA gradient match the oracle's step on those targets
    (with the regularisers off exp-6's loss is the multi-attribute step's with the one race attribute).  A second identical step from the
    same state gives a bit-identical gradient."""
    from oracle import fair_step as fs
    from finetune_fair_diffusion_amd.step import FairnessTrainer
    om = U.oracle_models(train_unet=True, train_te=False, lora_up_std=0.05, num_classes=6)
    pm = U.product_models(om["sds"], dev, train_unet=True, train_te=False, num_classes=6)
    thr = 0.5                  # drops one of the five targets (uncertainty 0.538); the plans of this batch survive +-5e-3 on every probability
    args = U.make_args(train_unet=True, train_text_encoder=False, uncertainty_threshold=thr, train_images_per_prompt_GPU=5, factor1=0.6,
                       factor2=0.3, face_race_confidence_level=0.9)
    tokens = U.tiny_tokens()
    B, S = 5, 3
    noises = torch.randn(B, 4, 32, 32, generator=torch.Generator().manual_seed(10))
    tg_o, u_o, img_o, probs_o = _oracle_race_targets(om, tokens, noises, S, thr)
    tr = FairnessTrainer(args, pm["text_encoder"], pm["unet"], pm["vae"], pm["classifier"], pm["scheduler"], eval_text_encoder=pm["eval_text_encoder"],
                         eval_unet=pm["eval_unet"], experiment="exp-6", device=dev)
    assert not tr.device_tail and tr.enumerated_targets and tr.ot_on_device
    grads = []

    def spy(N_backward, apply_=True):
        grads.append(tr.banks[0].grad.clone())
        return True
    tr.sync_and_update = spy
    out = tr.train_step(tokens, noises, S)
    err = float((out["images"].float().cpu() - img_o).abs().max() / img_o.abs().max())
    print(f"exp-6 R1 images rel err {err:.3e}; oracle probs {probs_o.tolist()}; uncertainties {u_o.tolist()}")
    assert err < 3e-2
    assert list(out["targets_by_attr"]) == ["race"]
    assert out["targets"].tolist() == tg_o.tolist(), (out["targets"], tg_o)
    assert int((tg_o != -1).sum()) >= 2          # the CE term is exercised
    assert out["uncertainty"].dtype == torch.float32
    print(f"exp-6: target phase {tr.last_ot_ms[0]:.2f} ms on the worker, main thread waited {tr.last_ot_ms[1]:.2f} ms; targets {tg_o.tolist()}")
    models_o = dict(text_encoder=om["text_encoder"], unet=om["unet"], vae=om["vae"], classifier=om["classifier"], scheduler=om["scheduler"])
    for p in om["lora_params"]:
        p.grad = None
    ref = fs.fairness_step_multi(models_o, tokens, noises, S, dict(train_GPU_batch_size=3, size_face=64), RACE, {"race": tg_o})
    lf, lr = out["loss_fair"], ref["losses"]["race"]
    assert ((lf == -1) == (lr == -1)).all()
    rel = float((lf - lr).abs().max() / lr.abs().max())
    print(f"exp-6 loss_fair rel err {rel:.3e}")
    assert rel < 2e-2
    names = list(om["unet_lora_layers"].state_dict().keys())
    refg = torch.cat([p.grad.flatten() for p in om["unet_lora_layers"].parameters()])
    got = torch.cat([tr.banks[0].view(n, grads[0]).flatten() for n in names])
    cos = float(F.cosine_similarity(got.cpu().double(), refg.double(), dim=0))
    ratio = float(got.norm().cpu() / refg.norm())
    print(f"cosine(exp-6 unet grads) = {cos}  norm ratio = {ratio}")
    assert cos > 0.97 and 0.8 < ratio < 1.25
    out2 = tr.train_step(tokens, noises, S)
    assert out2["targets"].tolist() == out["targets"].tolist()
    assert torch.equal(grads[1], grads[0]), "a second identical exp-6 step gave a different gradient"


def test_train_driver_exp6_full_loss_and_export(tmp_path):
    """The driver with every loss term on (synthetic weights, tiny configs): two exp-6 steps on the 6-logit head, all loss terms finite, a
    checkpoint written and exported."""
    from finetune_fair_diffusion_amd import checkpoint as ck
    from finetune_fair_diffusion_amd import train
    from finetune_fair_diffusion_amd.factory import TINY
    logs = []
    argv = ["--experiment", "exp-6", "--synthetic", "--train_unet", "--rank", "4", "--max_train_steps", "2", "--checkpointing_steps", "2",
            "--checkpointing_steps_long", "100", "--num_denoising_steps", "3", "--train_images_per_prompt_GPU", "4", "--train_GPU_batch_size", "3",
            "--val_GPU_batch_size", "4", "--img_size_small", "56", "--weight_loss_img", "6", "--weight_loss_face", "0.5", "--uncertainty_threshold", "1.0",
            "--output_dir", str(tmp_path)]
    tr, n = train.main(argv, cfgs=TINY, log=logs.append)
    recs = [json.loads(x) for x in logs]
    assert n == 2 and tr.experiment == "exp-6" and tr.use_img_loss and tr.use_face_loss and not tr.device_tail
    assert tr.clf.num_classes == 6 and tr.face_conf == 0.9 and tr.factors1 == [0.6] and tr.factors2 == [0.3]
    assert len(recs) == 2
    for r in recs:
        assert r["grad_is_finite"] and r["loss_CLIP"] is not None and r["loss_DINO"] is not None
        for k in ("loss_CLIP", "loss_DINO", "loss_face", "loss_fair"):
            assert r[k] is None or math.isfinite(r[k]), (k, r)
        assert 0 <= r["loss_CLIP"] < 2
    ckpt = tmp_path / "checkpoints" / "checkpoint_tmp-2"
    assert (ckpt / "unet_lora.pth").exists()
    out, files = ck.export_checkpoint(str(ckpt))
    assert "unet_lora.pth" in files and os.path.exists(os.path.join(out, "unet_lora.pth"))
