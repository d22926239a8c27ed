"""The plain fp64 statement of ``transformers.CLIPTextModelWithProjection(input_ids).text_embeds`` that the text-score tests compare against
(tests/test_textscore_cpu.py holds it to transformers itself; tests/test_textscore_gpu.py and tests/run_bf16_textscore_checks.py hold the kernels to
it).  It takes the transformers key names; exact ``gelu``; pooled at ``ids.argmax(-1)``: the end-of-text id is the largest of the vocabulary."""
import torch
import torch.nn.functional as F


def text_embeds_ref(sd, ids, heads, eps=1e-5):
    """sd: {transformers key: tensor}, ids [B,T] int64 -> text_embeds [B, projection_dim] float64."""
    w = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    B, T = ids.shape
    x = w["text_model.embeddings.token_embedding.weight"][ids] + w["text_model.embeddings.position_embedding.weight"][:T]
    D = x.shape[-1]
    d = D // heads
    mask = torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    i = 0
    while f"text_model.encoder.layers.{i}.layer_norm1.weight" in w:
        p = f"text_model.encoder.layers.{i}."
        lin = lambda t, n: F.linear(t, w[p + n + ".weight"], w[p + n + ".bias"])  # noqa: E731
        n1 = F.layer_norm(x, (D,), w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], eps)
        q, k, v = (lin(n1, f"self_attn.{n}_proj").view(B, T, heads, d).transpose(1, 2) for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, dim=-1) @ v
        x = x + lin(a.transpose(1, 2).reshape(B, T, D), "self_attn.out_proj")
        n2 = F.layer_norm(x, (D,), w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], eps)
        x = x + lin(F.gelu(lin(n2, "mlp.fc1")), "mlp.fc2")
        i += 1
    y = F.layer_norm(x, (D,), w["text_model.final_layer_norm.weight"], w["text_model.final_layer_norm.bias"], eps)
    return y[torch.arange(B), ids.argmax(-1)] @ w["text_projection.weight"].t()


def rows_with_eot_at(positions, vocab, T=77, seed=0, tail="pad"):
    """[len(positions), T] ids: begin (vocab-2), random words below it, the end-of-text id (vocab-1, the largest) at ``positions[r]``, and behind it
    id 0 (``tail="pad"``) or random words (``"random"``; never the end-of-text id) -- the same words in front of it either way."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab - 2, (len(positions), T), generator=g)
    behind = torch.randint(1, vocab - 2, (len(positions), T), generator=g)
    ids[:, 0] = vocab - 2
    for r, p in enumerate(positions):
        assert 1 <= p < T
        ids[r, p] = vocab - 1
        ids[r, p + 1:] = behind[r, p + 1:] if tail == "random" else 0
    return ids
