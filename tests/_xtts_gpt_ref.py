"""fp64 oracle of the XTTS GPT, ``torch.nn.functional`` only.

It has no KV cache: every step recomputes the whole sequence [cond | start_text, text, stop_text |
start_audio, codes so far], so it cannot share a cache bug with the library.  It holds the logits
processors in the HF order (repetition penalty, temperature, top-k, top-p, inverse-CDF draw), the
teacher-forced latent pass, and ``EagerGpt``, the same model in fp32 torch eager with a KV cache (the
baseline of scripts/xtts_gpt_bench.py).

A model is a dict ``cfg`` (layers, model_dim, heads, n_text, n_audio, start_text, stop_text, start_audio,
stop_audio, text_positions, mel_positions) and a state dict with the ``gpt.*`` checkpoint keys.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

EPS = 1e-5


def gelu_new(v: torch.Tensor) -> torch.Tensor:
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v**3)))


def _ln(x, sd, name):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], EPS)


def to64(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {k: v.detach().to("cpu", torch.float64) for k, v in sd.items()}


def trunk(sd, cfg, x: torch.Tensor) -> torch.Tensor:
    """x [T, E] input embeddings -> the hidden states after the last layer (before ln_f), causal."""
    T, E = x.shape
    H = cfg["heads"]
    dk = E // H
    mask = torch.ones(T, T, dtype=torch.bool).tril()
    for i in range(cfg["layers"]):
        p = f"gpt.h.{i}."
        h = _ln(x, sd, p + "ln_1")
        qkv = h @ sd[p + "attn.c_attn.weight"] + sd[p + "attn.c_attn.bias"]  # HF Conv1D: [in][out]
        q, k, v = (t.reshape(T, H, dk).transpose(0, 1) for t in qkv.split(E, dim=-1))
        s = (q @ k.transpose(1, 2)) / math.sqrt(dk)
        s = s.masked_fill(~mask, float("-inf"))
        a = (F.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(T, E)
        x = x + a @ sd[p + "attn.c_proj.weight"] + sd[p + "attn.c_proj.bias"]
        h = _ln(x, sd, p + "ln_2")
        h = gelu_new(h @ sd[p + "mlp.c_fc.weight"] + sd[p + "mlp.c_fc.bias"])
        x = x + h @ sd[p + "mlp.c_proj.weight"] + sd[p + "mlp.c_proj.bias"]
    return x


def normed(sd, h: torch.Tensor) -> torch.Tensor:
    """final_norm(ln_f(h)): both, in that order."""
    return _ln(_ln(h, sd, "gpt.ln_f"), sd, "final_norm")


def prefix_rows(sd, cfg, cond: torch.Tensor, text: Sequence[int]) -> torch.Tensor:
    t = torch.tensor([cfg["start_text"], *[int(v) for v in text], cfg["stop_text"]], dtype=torch.int64)
    emb = sd["text_embedding.weight"][t] + sd["text_pos_embedding.emb.weight"][: len(t)]
    return torch.cat([cond.to(torch.float64), emb], dim=0)


def mel_rows(sd, cfg, tokens: Sequence[int]) -> torch.Tensor:
    t = torch.tensor([int(v) for v in tokens], dtype=torch.int64)
    return sd["mel_embedding.weight"][t] + sd["mel_pos_embedding.emb.weight"][: len(t)]


def mel_pass(sd, cfg, cond, text, mel_tokens: Sequence[int]):
    """One causal pass over [prefix | mel_tokens]: (final_norm(ln_f(h)) [n, E], mel_head logits [n, V]) at the
    mel positions."""
    pre = prefix_rows(sd, cfg, cond, text)
    x = torch.cat([pre, mel_rows(sd, cfg, mel_tokens)], dim=0)
    lat = normed(sd, trunk(sd, cfg, x)[pre.shape[0]:])
    return lat, lat @ sd["mel_head.weight"].T + sd["mel_head.bias"]


def penalise(l: torch.Tensor, ids, penalty: float) -> torch.Tensor:
    l = l.clone()
    idx = torch.tensor(sorted({int(i) for i in ids}), dtype=torch.int64)
    sel = l[idx]
    l[idx] = torch.where(sel < 0, sel * penalty, sel / penalty)
    return l


def process(logits: torch.Tensor, ids, penalty=1.0, temperature=1.0, top_k=0, top_p=1.0, u: Optional[float] = None):
    """One logits -> token step.  ids: the penalised id set.  Returns (token, info) with the margins the
    GPU tests' conditions are stated on: greedy_gap (top-2 gap after the penalty), topk_gap (k-th against
    (k+1)-th logit), topp_gap (the top-p cumulative against its threshold), u_gap (u against the CDF
    edges)."""
    l = penalise(logits.to(torch.float64), ids, penalty)
    V = l.numel()
    info = {}
    if u is None:
        top2 = torch.topk(l, 2).values
        info["greedy_gap"] = float(top2[0] - top2[1])
        return int(torch.nonzero(l == l.max())[0]), info  # the lowest id on ties
    l = l / temperature
    if 0 < top_k < V:
        vals = torch.topk(l, top_k + 1).values
        info["topk_gap"] = float(vals[top_k - 1] - vals[top_k])
        l = l.masked_fill(l < vals[top_k - 1], float("-inf"))
    if top_p < 1.0:
        sl, si = torch.sort(l, stable=True)
        c = torch.cumsum(F.softmax(sl, dim=-1), dim=-1)
        remove = c <= 1.0 - top_p
        remove[-1] = False  # always keep one
        fin = torch.isfinite(sl)
        info["topp_gap"] = float((c[fin] - (1.0 - top_p)).abs().min())
        l = l.clone()
        l[si[remove]] = float("-inf")
    p = F.softmax(l, dim=-1)
    cdf = torch.cumsum(p, dim=-1)
    info["u_gap"] = float((cdf[p > 0] - u).abs().min())
    hit = torch.nonzero(cdf > u)
    return (int(hit[0]) if hit.numel() else int(torch.nonzero(p > 0)[-1])), info


def generate(sd, cfg, cond, text, max_new: int, penalty=1.0, temperature=1.0, top_k=0, top_p=1.0,
             u: Optional[Sequence[float]] = None):
    """Free run of one utterance.  Returns dict(codes [n], n, logits [n, V], latents [n, E], infos)."""
    mel = [cfg["start_audio"]]
    codes: List[int] = []
    logits, lats, infos = [], [], []
    for s in range(max_new):
        lat, lg = mel_pass(sd, cfg, cond, text, mel)
        ids = [1, cfg["start_audio"], *codes]
        tok, info = process(lg[-1], ids, penalty, temperature, top_k, top_p, None if u is None else float(u[s]))
        logits.append(lg[-1])
        lats.append(lat[-1])
        infos.append(info)
        codes.append(tok)
        mel.append(tok)
        if tok == cfg["stop_audio"]:
            break
    return {"codes": codes, "n": len(codes), "logits": torch.stack(logits), "latents": torch.stack(lats),
            "infos": infos}


def teacher_forced(sd, cfg, cond, text, codes: Sequence[int]):
    """The pass over [start_audio, codes, stop_audio]: (latents [n + 2, E], logits [n + 2, V])."""
    return mel_pass(sd, cfg, cond, text, [cfg["start_audio"], *codes, cfg["stop_audio"]])


def latents(sd, cfg, cond, text, codes: Sequence[int]) -> torch.Tensor:
    """return_latent=True: the n + 2 mel positions without the last 4 -> [n - 2, E]."""
    return teacher_forced(sd, cfg, cond, text, codes)[0][:-4]


def incremental_logits(sd, cfg, cond, text, codes: Sequence[int]) -> torch.Tensor:
    """Logits of the steps 0 .. len(codes) computed one growing sequence at a time, [len(codes) + 1, V]."""
    mel = [cfg["start_audio"]]
    out = []
    for s in range(len(codes) + 1):
        out.append(mel_pass(sd, cfg, cond, text, mel)[1][-1])
        if s < len(codes):
            mel.append(codes[s])
    return torch.stack(out)


class EagerGpt:
    """The same model in torch eager (fp32 by default) with a KV cache, on any device: the baseline the
    bench compares the library's step with.  Greedy, stop disabled."""

    def __init__(self, sd, cfg, device, dtype=torch.float32):
        self.cfg = cfg
        self.sd = {k: v.detach().to(device=device, dtype=dtype) for k, v in sd.items()}
        self.dev, self.dtype = device, dtype

    def _layers(self, x, cache, pos):
        """x [B, T, E] new rows at positions [pos, pos + T); cache: per layer (k, v) [B, H, cap, dk]."""
        sd, cfg = self.sd, self.cfg
        B, T, E = x.shape
        H = cfg["heads"]
        dk = E // H
        for i in range(cfg["layers"]):
            p = f"gpt.h.{i}."
            h = F.layer_norm(x, (E,), sd[p + "ln_1.weight"], sd[p + "ln_1.bias"], EPS)
            qkv = torch.addmm(sd[p + "attn.c_attn.bias"], h.reshape(B * T, E), sd[p + "attn.c_attn.weight"])
            q, k, v = (t.reshape(B, T, H, dk).transpose(1, 2) for t in qkv.split(E, dim=-1))
            kc, vc = cache[i]
            kc[:, :, pos:pos + T] = k
            vc[:, :, pos:pos + T] = v
            s = (q @ kc[:, :, :pos + T].transpose(2, 3)) / math.sqrt(dk)
            if T > 1:
                m = torch.ones(T, pos + T, dtype=torch.bool, device=x.device).tril(pos)
                s = s.masked_fill(~m, float("-inf"))
            a = (F.softmax(s, dim=-1) @ vc[:, :, :pos + T]).transpose(1, 2).reshape(B * T, E)
            x = x + torch.addmm(sd[p + "attn.c_proj.bias"], a, sd[p + "attn.c_proj.weight"]).reshape(B, T, E)
            h = F.layer_norm(x, (E,), sd[p + "ln_2.weight"], sd[p + "ln_2.bias"], EPS)
            h = gelu_new(torch.addmm(sd[p + "mlp.c_fc.bias"], h.reshape(B * T, E), sd[p + "mlp.c_fc.weight"]))
            x = x + torch.addmm(sd[p + "mlp.c_proj.bias"], h, sd[p + "mlp.c_proj.weight"]).reshape(B, T, E)
        return x

    @torch.no_grad()
    def generate(self, cond, text, steps: int):
        """cond [B, P, E], text [B, T] (every token valid) -> greedy codes [B, steps] (penalty 1)."""
        sd, cfg = self.sd, self.cfg
        B, T = text.shape
        E = cfg["model_dim"]
        H = cfg["heads"]
        t = torch.cat([torch.full((B, 1), cfg["start_text"], device=self.dev), text.to(self.dev),
                       torch.full((B, 1), cfg["stop_text"], device=self.dev)], dim=1)
        pre = torch.cat([cond.to(self.dev, self.dtype),
                         sd["text_embedding.weight"][t] + sd["text_pos_embedding.emb.weight"][: T + 2]], dim=1)
        cap = pre.shape[1] + steps
        cache = [(torch.zeros(B, H, cap, E // H, device=self.dev, dtype=self.dtype),
                  torch.zeros(B, H, cap, E // H, device=self.dev, dtype=self.dtype)) for _ in range(cfg["layers"])]
        self._layers(pre, cache, 0)
        pos = pre.shape[1]
        tok = torch.full((B,), cfg["start_audio"], device=self.dev)
        codes = []
        for s in range(steps):
            x = (sd["mel_embedding.weight"][tok] + sd["mel_pos_embedding.emb.weight"][s]).unsqueeze(1)
            h = self._layers(x, cache, pos + s)[:, 0]
            h = F.layer_norm(h, (E,), sd["gpt.ln_f.weight"], sd["gpt.ln_f.bias"], EPS)
            h = F.layer_norm(h, (E,), sd["final_norm.weight"], sd["final_norm.bias"], EPS)
            tok = torch.addmm(sd["mel_head.bias"], h, sd["mel_head.weight"].T).argmax(dim=-1)
            codes.append(tok)
        return torch.stack(codes, dim=1)
