"""XTTS GPT without a device: the module's parameter tree, the checkpoint filter, the ABI's weight inventory
and validation, the excluded options, the oracle's self-consistency, the conditions the GPU tests' cases
meet (checked on the oracle alone), and the packers under AddressSanitizer + UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _xtts_gpt_cases as C
import _xtts_gpt_ref as R
from tts_amd import _native as N
from tts_amd.tts import Xtts, XttsGPT
from tts_amd.tts.xtts_gpt import gpt_checkpoint_filter

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-3_amd")


def expected_keys(cfg: dict):
    E = cfg["model_dim"]
    keys = {
        "text_embedding.weight": (cfg["n_text"], E),
        "mel_embedding.weight": (cfg["n_audio"], E),
        "text_pos_embedding.emb.weight": (cfg["text_positions"], E),
        "mel_pos_embedding.emb.weight": (cfg["mel_positions"], E),
        "gpt.ln_f.weight": (E,), "gpt.ln_f.bias": (E,),
        "final_norm.weight": (E,), "final_norm.bias": (E,),
        "text_head.weight": (cfg["n_text"], E), "text_head.bias": (cfg["n_text"],),
        "mel_head.weight": (cfg["n_audio"], E), "mel_head.bias": (cfg["n_audio"],),
    }
    for i in range(cfg["layers"]):
        p = f"gpt.h.{i}."
        for ln in ("ln_1", "ln_2"):
            keys[p + ln + ".weight"] = (E,)
            keys[p + ln + ".bias"] = (E,)
        keys[p + "attn.c_attn.weight"] = (E, 3 * E)  # HF Conv1D: [in][out]
        keys[p + "attn.c_attn.bias"] = (3 * E,)
        keys[p + "attn.c_proj.weight"] = (E, E)
        keys[p + "attn.c_proj.bias"] = (E,)
        keys[p + "mlp.c_fc.weight"] = (E, 4 * E)
        keys[p + "mlp.c_fc.bias"] = (4 * E,)
        keys[p + "mlp.c_proj.weight"] = (4 * E, E)
        keys[p + "mlp.c_proj.bias"] = (E,)
    return keys


def build(name: str, **kw) -> XttsGPT:
    return XttsGPT(**C.ctor_kwargs(C.MODELS[name]), math_mode="fp32", **kw)


@pytest.mark.parametrize("name", list(C.MODELS))
def test_state_dict_keys(name):
    cfg = C.MODELS[name]
    m = build(name)
    keys = expected_keys(cfg)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == keys
    sd = C.state_dict(cfg, C.MODEL_SEED[name])
    assert {k: tuple(v.shape) for k, v in sd.items()} == keys
    m.load_state_dict(sd, strict=True)


def test_conv1d_weight_reaches_the_library_as_stored():
    """A c_attn weight with one nonzero entry at [in = 3][out = 5]: the array handed to the library is the
    stored [in][out] buffer, not a transpose (the packer reads that layout; tests_native/gpt_pack_check.cpp
    places the same entry in the packed image)."""
    m = build("narrow")
    E = m.model_dim
    with torch.no_grad():
        m.gpt.h[0].attn.c_attn.weight.zero_()
        m.gpt.h[0].attn.c_attn.weight[3, 5] = 2.5
    w = m._weight_list()[4 + 2]
    assert w.shape == (E, 3 * E) and w.flags["C_CONTIGUOUS"]
    assert np.flatnonzero(w.reshape(-1)).tolist() == [3 * 3 * E + 5] and w[3, 5] == 2.5


def test_load_checkpoint_drops_the_unused_keys(tmp_path):
    cfg = C.MODELS["narrow"]
    sd = C.state_dict(cfg, C.MODEL_SEED["narrow"])
    full = {"gpt." + k: v for k, v in sd.items()}
    extra = ["conditioning_encoder.init.weight", "conditioning_perceiver.latents", "gpt_inference.transformer.h.0.ln_1.weight",
             "gpt.h.0.attn.bias", "gpt.h.1.attn.masked_bias", "mel_layer_pos_embedding.emb.weight",
             "text_layer_pos_embedding.emb.weight"]
    for k in extra:
        full["gpt." + k] = torch.zeros(2, 2)
    full["hifigan_decoder.waveform_decoder.conv_pre.weight"] = torch.zeros(1)
    assert set(gpt_checkpoint_filter({k: 0 for k in list(sd) + extra})) == set(sd)
    path = tmp_path / "ckpt.pth"
    torch.save({"model": full}, path)
    m = build("narrow")
    m.train()
    m.load_checkpoint(str(path), eval=True)
    assert not m.training
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("name", list(C.MODELS))
def test_abi_weight_inventory(name):
    m = build(name)
    ws = m._weight_list()
    cfg = m._make_cfg(C.MODELS[name]["P"])
    lib = N.lib()
    assert lib.tts_xtts_gpt_num_weights(ctypes.byref(cfg)) == len(ws) == 4 + 12 * C.MODELS[name]["layers"] + 6
    for i, w in enumerate(ws):
        assert lib.tts_xtts_gpt_weight_numel(ctypes.byref(cfg), i) == w.size, i
    assert lib.tts_xtts_gpt_weight_numel(ctypes.byref(cfg), len(ws)) == -1
    assert lib.tts_abi_version() == 115
    assert lib.tts_op_gpt_decode_attn_waves() >= 1


def test_every_new_symbol_is_exported():
    lib = N.lib()
    for name in N.SIGNATURES:
        if "xtts_gpt" in name or "op_gpt" in name or name == "tts_op_mha_causal":
            assert hasattr(lib, name), name


def test_excluded_options_raise():
    m = build("narrow")
    cond, text = C.inputs(C.MODELS["narrow"], 1, 1, 4)
    for kw in (dict(num_beams=2), dict(input_tokens=torch.zeros(1, 2, dtype=torch.int64)), dict(return_attentions=True)):
        with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
            m.generate(cond, text, **kw)
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        m.forward(text, None, torch.zeros(1, 6, dtype=torch.int64), torch.tensor([6 * 1024]), cond_latents=cond,
                  return_attentions=True)
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        m.forward(text, None, torch.zeros(1, 6, dtype=torch.int64), torch.tensor([6 * 1024]), cond_latents=cond,
                  return_latent=False)
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        XttsGPT(**C.ctor_kwargs(C.MODELS["narrow"]), train_solo_embeddings=True)
    x = Xtts(m, None)
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        x.inference(text, cond, torch.zeros(1, 8, 1), num_beams=4)


def test_token_ids_outside_their_tables_raise_on_the_host():
    m = build("narrow")
    cfg = C.MODELS["narrow"]
    cond, text = C.inputs(cfg, 1, 1, 4)
    bad = text.clone()
    bad[0, 2] = cfg["n_text"]
    with pytest.raises(IndexError, match="text token ids"):
        m.generate(cond, bad)
    with pytest.raises(IndexError, match="text token ids"):
        m.generate(cond, -text)
    with pytest.raises(IndexError, match="audio codes"):
        m.forward(text, None, torch.tensor([[3, cfg["n_audio"], 4, 5]]), None, cond_latents=cond,
                  code_lengths=torch.tensor([4]))


def cfg_of(**over):
    c = build("narrow")._make_cfg(5)
    for k, v in over.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("over,status,msg", [
    (dict(layers=0), N.TTS_ERR_INVALID, "layers, model_dim, heads"),
    (dict(heads=3), N.TTS_ERR_INVALID, "layers, model_dim, heads"),
    (dict(start_audio_token=67), N.TTS_ERR_INVALID, "outside the audio table"),
    (dict(stop_text_token=-1), N.TTS_ERR_INVALID, "outside the text table"),
    (dict(mel_positions=0), N.TTS_ERR_INVALID, "position counts"),
    (dict(chunk=-1), N.TTS_ERR_INVALID, "chunk"),
    (dict(math_mode=9), N.TTS_ERR_INVALID, "math_mode"),
    (dict(heads=8), N.TTS_ERR_UNSUPPORTED, "head size must be 32, 64 or 128"),      # dk 16
    (dict(model_dim=96, heads=3), N.TTS_ERR_UNSUPPORTED, "multiple of 64"),         # dk 32, E % 64 != 0
    (dict(n_audio_tokens=8195), N.TTS_ERR_UNSUPPORTED, "at most 8194 audio tokens"),
])
def test_cfg_validation(over, status, msg):
    lib = N.lib()
    c = cfg_of(**over)
    assert lib.tts_xtts_gpt_num_weights(ctypes.byref(c)) == -status
    assert msg in lib.tts_last_error().decode()
    assert lib.tts_xtts_gpt_weight_numel(ctypes.byref(c), 0) == -1


def test_cfg_limits_accept_their_edges():
    lib = N.lib()
    assert lib.tts_xtts_gpt_num_weights(ctypes.byref(cfg_of(n_audio_tokens=8194, start_audio_token=8192,
                                                           stop_audio_token=8193))) > 0
    for heads in (1, 2, 4):  # dk 128, 64, 32
        assert lib.tts_xtts_gpt_num_weights(ctypes.byref(cfg_of(heads=heads))) > 0


# ------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", ["narrow", "narrow32"])
def test_oracle_incremental_equals_one_pass(name):
    cfg = C.MODELS[name]
    sd = R.to64(C.state_dict(cfg, C.MODEL_SEED[name]))
    cond, text = C.inputs(cfg, 5, 1, 6)
    codes = [3, 17, 64, 2, 2, 40, 9]
    inc = R.incremental_logits(sd, cfg, cond[0], text[0].tolist(), codes)
    lat, one = R.mel_pass(sd, cfg, cond[0], text[0].tolist(), [cfg["start_audio"], *codes])
    assert inc.shape == one.shape == (len(codes) + 1, cfg["n_audio"])
    assert float((inc - one).abs().max()) <= 1e-12
    # the latent pass's trimming rule: n + 2 positions without the last 4
    assert R.latents(sd, cfg, cond[0], text[0].tolist(), codes).shape == (len(codes) - 2, cfg["model_dim"])
    assert float((R.latents(sd, cfg, cond[0], text[0].tolist(), codes) - lat[: len(codes) - 2]).abs().max()) <= 1e-12


def test_oracle_processors_on_a_hand_case():
    l = torch.tensor([2.0, 1.0, 0.5, -1.0, 0.0])
    # penalty 2 over {1, 3}: 1.0 -> 0.5, -1.0 -> -2.0; greedy takes id 0
    tok, info = R.process(l, [1, 3], penalty=2.0)
    assert tok == 0 and abs(info["greedy_gap"] - 1.5) < 1e-12
    # an exact tie: the lowest id
    assert R.process(torch.tensor([1.0, 3.0, 3.0]), [0], penalty=1.0)[0] == 1
    # top-k 2 keeps ids 0, 1; p = softmax([2, 1]) = [0.731, 0.269]; u = 0.8 falls on id 1
    assert R.process(l, [], 1.0, 1.0, 2, 1.0, 0.8)[0] == 1
    assert R.process(l, [], 1.0, 1.0, 2, 1.0, 0.7)[0] == 0
    # top-p 0.5: ascending cumulative <= 0.5 goes, which leaves id 0 alone (p0 = 0.574 of the five)
    assert R.process(l, [], 1.0, 1.0, 0, 0.5, 0.99)[0] == 0


# ---------------------------------------------------------- conditions of the GPU tests, on the oracle
@pytest.mark.parametrize("case", list(C.FREE_RUN))
def test_greedy_margin_of_every_free_run_step(case):
    model, seed, B, T, lens, steps, pen = C.FREE_RUN[case]
    cfg = C.MODELS[model]
    sd = R.to64(C.state_dict(cfg, C.MODEL_SEED[model]))
    cond, text = C.inputs(cfg, seed, B, T)
    for b in range(B):
        L = T if lens is None else lens[b]
        out = R.generate(sd, cfg, cond[b], text[b, :L].tolist(), steps, penalty=pen)
        gaps = [i["greedy_gap"] for i in out["infos"]]
        assert len(gaps) == out["n"] and min(gaps) >= C.MARGIN, (case, b, min(gaps))
        assert float(out["logits"].std()) > 0.5  # the logits spread by O(1)


def test_greedy_margin_of_the_empty_prefix_case():
    cfg = C.MODELS["narrow"]
    sd = R.to64(C.state_dict(cfg, C.MODEL_SEED["narrow"]))
    out = R.generate(sd, cfg, torch.zeros(0, cfg["model_dim"]), [], 5, penalty=10.0)
    assert out["n"] == 5 and min(i["greedy_gap"] for i in out["infos"]) >= C.MARGIN


def test_stop_case_ends_at_three_different_steps_with_margin():
    s = C.STOP_CASE
    cfg = C.MODELS[s["model"]]
    sd = R.to64(C.stop_state_dict())
    cond, text = C.inputs(cfg, s["seed"], s["B"], s["T"])
    ns = []
    for b in range(s["B"]):
        out = R.generate(sd, cfg, cond[b], text[b, : s["lens"][b]].tolist(), s["steps"], penalty=s["penalty"])
        assert min(i["greedy_gap"] for i in out["infos"]) >= C.MARGIN
        assert out["codes"][-1] == cfg["stop_audio"]
        ns.append(out["n"])
    assert ns == s["n"] and len(set(ns)) == 3 and max(ns) < s["steps"]


def test_draw_margins_of_every_step_of_the_sampled_run():
    s = C.SAMPLED_RUN
    cfg = C.MODELS[s["model"]]
    sd = R.to64(C.state_dict(cfg, C.MODEL_SEED[s["model"]]))
    cond, text = C.inputs(cfg, s["seed"], s["B"], s["T"])
    u = C.sampled_run_uniforms()
    for b in range(s["B"]):
        out = R.generate(sd, cfg, cond[b], text[b].tolist(), s["steps"], s["penalty"], s["temperature"], s["top_k"],
                         s["top_p"], u[b].tolist())
        for step, info in enumerate(out["infos"]):
            for name, gap in info.items():
                assert gap >= C.MARGIN, (b, step, name, gap)


@pytest.mark.parametrize("V", C.SAMPLE_V)
def test_draw_margins_of_every_sample_case(V):
    logits, prev, u = C.sample_case(V)
    for (k, p, pen, temp) in C.sample_combos(V):
        for b in range(logits.shape[0]):
            ids = [1, V - 2, *prev[b].tolist()]
            _, info = R.process(logits[b], ids, pen, temp, k, p, float(u[b]))
            assert ("topk_gap" in info) == (k < V) and ("topp_gap" in info) == (p < 1.0)
            for name, gap in info.items():
                assert gap >= C.MARGIN, (V, k, p, pen, temp, b, name, gap)
            _, info = R.process(logits[b], ids, pen)
            assert info["greedy_gap"] >= C.MARGIN


# ------------------------------------------------------------------------------------ the packers
@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/llvm/bin/clang++"),
                    reason="needs make and the ROCm clang++")
def test_gpt_packers_clean_under_asan_ubsan():
    r = subprocess.run(["make", "-C", PKG, "asan-check-gpt"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "GPT packers OK" in r.stdout
