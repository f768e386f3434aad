"""Tacotron2 without a device: the module's parameter tree, the ABI's weight inventory and validation,
the excluded options, the oracle's self-consistency, and the conditions the GPU tests' inputs meet."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _tacotron2_cases as C
import _tacotron2_ref as R
from _util import max_abs, rel_rms, tol
from tts_amd import _native as N
from tts_amd.tts import Tacotron2, Tacotron2Args


def expected_keys(a: dict, D: int):
    E, Q, P, A, F, K = (a[k] for k in ("encoder_dim", "query_dim", "prenet_dim", "attention_dim", "location_filters",
                                        "location_kernel_size"))
    C_, r = a["out_channels"], a["r"]
    keys = {"embedding.weight": (a["num_chars"], E)}

    def conv_bn(pre, co, ci):
        keys[pre + "convolution1d.weight"] = (co, ci, 5)
        keys[pre + "convolution1d.bias"] = (co,)
        for n in ("weight", "bias", "running_mean", "running_var"):
            keys[pre + "batch_normalization." + n] = (co,)
        keys[pre + "batch_normalization.num_batches_tracked"] = ()

    for i in range(3):
        conv_bn(f"encoder.convolutions.{i}.", E, E)
    for sfx in ("", "_reverse"):
        keys[f"encoder.lstm.weight_ih_l0{sfx}"] = (2 * E, E)
        keys[f"encoder.lstm.weight_hh_l0{sfx}"] = (2 * E, E // 2)
        keys[f"encoder.lstm.bias_ih_l0{sfx}"] = (2 * E,)
        keys[f"encoder.lstm.bias_hh_l0{sfx}"] = (2 * E,)
    keys["decoder.prenet.linear_layers.0.linear_layer.weight"] = (P, C_)
    keys["decoder.prenet.linear_layers.1.linear_layer.weight"] = (P, P)
    for name, I in (("attention_rnn", P + D), ("decoder_rnn", Q + D)):
        keys[f"decoder.{name}.weight_ih"] = (4 * Q, I)
        keys[f"decoder.{name}.weight_hh"] = (4 * Q, Q)
        keys[f"decoder.{name}.bias_ih"] = (4 * Q,)
        keys[f"decoder.{name}.bias_hh"] = (4 * Q,)
    keys["decoder.attention.query_layer.linear_layer.weight"] = (A, Q)
    keys["decoder.attention.inputs_layer.linear_layer.weight"] = (A, D)
    keys["decoder.attention.v.linear_layer.weight"] = (1, A)
    keys["decoder.attention.v.linear_layer.bias"] = (1,)
    keys["decoder.attention.location_layer.location_conv1d.weight"] = (F, 2, K)
    keys["decoder.attention.location_layer.location_dense.linear_layer.weight"] = (A, F)
    keys["decoder.linear_projection.linear_layer.weight"] = (C_ * r, Q + D)
    keys["decoder.linear_projection.linear_layer.bias"] = (C_ * r,)
    keys["decoder.stopnet.1.linear_layer.weight"] = (1, Q + C_ * r)
    keys["decoder.stopnet.1.linear_layer.bias"] = (1,)
    dims = [C_, 512, 512, 512, 512, C_]
    for i in range(5):
        conv_bn(f"postnet.convolutions.{i}.", dims[i + 1], dims[i])
    return keys


@pytest.mark.parametrize("name,D", [("reference", 512), ("narrow", 64 + 16), ("narrow_dvec", 64 + 12)])
def test_state_dict_keys(name, D):
    a = C.model_args(name)
    m = Tacotron2(a)
    keys = expected_keys(a, D)
    if a["use_speaker_embedding"]:
        keys["speaker_embedding.weight"] = (a["num_speakers"], a["speaker_embedding_dim"])
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == keys
    sd = C.state_dict(name)
    assert {k: tuple(v.shape) for k, v in sd.items()} == keys
    m.load_state_dict(sd, strict=True)


def test_reference_speaker_embedding_is_512_wide():
    m = Tacotron2(dict(C.MODELS["reference"], use_speaker_embedding=True, num_speakers=4))
    assert m.state_dict()["speaker_embedding.weight"].shape == (4, 512)
    assert m.state_dict()["decoder.attention.inputs_layer.linear_layer.weight"].shape == (128, 1024)


def test_load_checkpoint_drops_coarse_decoder(tmp_path):
    a = C.model_args("narrow")
    sd = dict(C.state_dict("narrow"))
    sd["coarse_decoder.prenet.linear_layers.0.linear_layer.weight"] = torch.zeros(3, 3)
    sd["coarse_decoder.stopnet.1.linear_layer.bias"] = torch.zeros(1)
    path = tmp_path / "ckpt.pth"
    torch.save({"model": sd}, path)
    m = Tacotron2(a)
    m.train()
    m.load_checkpoint(None, str(path), eval=True)
    assert not m.training
    assert torch.equal(m.embedding.weight, C.state_dict("narrow")["embedding.weight"])


@pytest.mark.parametrize("name", ["narrow", "narrow_dvec", "reference"])
def test_abi_weight_inventory(name):
    m = Tacotron2(C.model_args(name, r=3))
    ws = m._weight_list()
    lib = N.lib()
    assert lib.tts_tacotron2_num_weights(ctypes.byref(m._cfg)) == len(ws)
    for i, w in enumerate(ws):
        assert lib.tts_tacotron2_weight_numel(ctypes.byref(m._cfg), i) == w.size, i
    assert lib.tts_tacotron2_weight_numel(ctypes.byref(m._cfg), len(ws)) == -1
    assert lib.tts_abi_version() == 115


@pytest.mark.parametrize("kw", [dict(attention_type="graves"), dict(attention_type="dynamic_convolution"),
                                dict(location_attn=False), dict(windowing=True), dict(use_forward_attn=True),
                                dict(transition_agent=True), dict(prenet_type="bn"),
                                dict(prenet_dropout_at_inference=True), dict(use_gst=True),
                                dict(use_capacitron_vae=True)])
def test_excluded_options_raise(kw):
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        Tacotron2(dict(C.model_args("narrow"), **kw))


def cfg_of(**over):
    c = Tacotron2(C.model_args("narrow"))._cfg
    for k, v in over.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("over,status", [
    (dict(), 0),
    (dict(encoder_dim=66), N.TTS_ERR_UNSUPPORTED),   # E / 2 = 33: not a multiple of the unit block
    (dict(query_dim=98), N.TTS_ERR_UNSUPPORTED),
    (dict(attention_dim=129), N.TTS_ERR_UNSUPPORTED),
    (dict(location_filters=33), N.TTS_ERR_UNSUPPORTED),
    (dict(location_kernel_size=33), N.TTS_ERR_UNSUPPORTED),
    (dict(location_kernel_size=30), N.TTS_ERR_UNSUPPORTED),
    (dict(query_dim=2052), N.TTS_ERR_UNSUPPORTED),
    (dict(prenet_dim=1025), N.TTS_ERR_UNSUPPORTED),
    (dict(r=52), N.TTS_ERR_UNSUPPORTED),             # 20 * 52 = 1040 outputs per step
    (dict(num_chars=0), N.TTS_ERR_INVALID),
    (dict(r=0), N.TTS_ERR_INVALID),
    (dict(encoder_dim=63), N.TTS_ERR_INVALID),
    (dict(attention_norm=2), N.TTS_ERR_INVALID),
    (dict(num_speakers=2, embed_dim=0), N.TTS_ERR_INVALID),
    (dict(math_mode=9), N.TTS_ERR_INVALID),
])
def test_config_validation(over, status):
    n = N.lib().tts_tacotron2_num_weights(ctypes.byref(cfg_of(**over)))
    if status == 0:
        assert n > 0
    else:
        assert n == -status and N.lib().tts_last_error()
    assert N.LSTM_UNIT_BLOCK == 4 and N.TACOTRON2_MAX_BATCH == 32


def test_cpu_module_refuses_to_run():
    m = Tacotron2(C.model_args("narrow"))
    m.load_state_dict(C.state_dict("narrow"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(torch.ones(1, 5, dtype=torch.int64), {"speaker_ids": torch.tensor([0])})
    from tts_amd.tts import lstm_cell
    with pytest.raises(RuntimeError):
        lstm_cell(torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(16, 4), torch.zeros(16, 4),
                  torch.zeros(16), torch.zeros(16))


# ------------------------------------------------------------------ oracle self-checks
def test_oracle_b1_equals_full_length_batch():
    a, sd = C.model_args("narrow"), C.state_dict("narrow")
    tok = C.tokens(3, 11, seed=2)
    spk = torch.tensor(C.SPEAKERS[:3])
    full = R.inference(sd, a, tok, x_lengths=torch.full((3,), 11), speaker_ids=spk, stop_threshold=2.0,
                       max_decoder_steps=5)
    for b in range(3):
        one = R.inference(sd, a, tok[b : b + 1], speaker_ids=spk[b : b + 1], stop_threshold=2.0, max_decoder_steps=5)
        for k in ("model_outputs", "decoder_outputs", "alignments", "stop_tokens"):
            assert max_abs(one[k][0], full[k][b]) < 1e-12, (k, b)


def test_oracle_packed_bilstm_equals_single_runs():
    sd = C.state_dict("narrow")
    tok = C.tokens(3, 11, seed=2)
    lens = torch.tensor([11, 6, 1])
    with torch.no_grad():
        enc = R.encoder(sd, tok, lens)
        for b in range(3):
            n = int(lens[b])
            # the convs see the padded tokens (the reference runs them before packing); the biLSTM does not
            x = torch.nn.functional.embedding(tok[b : b + 1], sd["embedding.weight"].double()).transpose(1, 2)
            for i in range(3):
                x = torch.relu(R._conv_bn(sd, f"encoder.convolutions.{i}.", x, torch.float64, None, ""))
            alone = R._lstm(sd, "encoder.lstm.", 64, torch.float64)(x.transpose(1, 2)[:, :n])[0]
            assert max_abs(enc[b, :n], alone[0]) < 1e-12
            assert float(enc[b, n:].abs().max()) == 0.0 if n < 11 else True


def test_oracle_counts_macs():
    counter = {}
    tok, kw = C.case_inputs("few_s2_r2_sigmoid")
    R.inference(C.state_dict("narrow"), C.model_args("narrow"), tok, **kw, stop_threshold=2.0, max_decoder_steps=2,
                counter=counter)
    assert counter["encoder.convs"] == 2 * 13 * 3 * 64 * 64 * 5
    assert counter["decoder.steps"] > 0 and counter["postnet"] > 0 and counter["encoder.lstm"] > 0


# ------------------------------------------------------------------ the GPU tests' input conditions
def entropy_ratio(name):
    a = C.reference(name)["alignments"]
    lengths = C.CASES[name][6]
    L = torch.tensor(lengths, dtype=torch.float64)
    ent = -(a * torch.log(a.clamp_min(1e-300))).sum(-1)
    return ent / torch.log(L)[:, None]


@pytest.mark.parametrize("name", ["free", "free_softmax", "free_dvec"])
def test_free_run_alignments_neither_uniform_nor_one_hot(name):
    """Over the 40 free-running steps the alignment entropy stays between 0.2 and 0.98 of log(length) after
    the first steps (step 0 reads all-zero attention weights), the largest weight below 0.9, and the stop
    probabilities lie on both sides of 0.5."""
    ref = C.reference(name)
    e = entropy_ratio(name)[:, 3:]
    assert 0.2 < float(e.min()) and float(e.max()) < 0.98, (float(e.min()), float(e.max()))
    assert float(ref["alignments"].max()) < 0.9
    p = ref["stop_tokens"]
    assert float(p.min()) < 0.5 < float(p.max())
    assert ref["decoder_outputs"].shape == (3, 80, 20)


def analogue_inside_half_gates(name, arith, mode):
    ref, got = C.reference(name), C.reference(name, arith)
    g = tol(mode)
    worst = {k: (max_abs(got[k], ref[k]), rel_rms(got[k], ref[k]))
             for k in ("model_outputs", "decoder_outputs", "alignments", "stop_tokens")}
    ok = all(ma <= g["max_abs_tol"] / 2 and rr <= g["rel_rms_tol"] / 2 for ma, rr in worst.values())
    return ok, worst


@pytest.mark.parametrize("name", sorted(C.FP32_GATED))
def test_cpu_analogue_decides_the_gates(name):
    """The device is held to the gates on the long cases only where torch's own CPU evaluation of the
    oracle in that arithmetic stays inside half of them; the recorded decisions match the measurement."""
    ok32, w32 = analogue_inside_half_gates(name, "fp32", "fp32")
    assert ok32 == C.FP32_GATED[name], w32
    ok16, w16 = analogue_inside_half_gates(name, "bf16w", "bf16")
    assert ok16 == C.BF16_GATED[name], w16


def test_stop_case_conditions():
    thr, steps = C.stop_threshold()
    p = C.reference("stop_probe")["stop_tokens"]
    S = C.STOP_STEPS
    stopped = sorted({s for s in steps if s < S})
    assert len(stopped) >= 2 and min(stopped) >= 2, steps      # (a) two different stop steps t >= 1
    assert steps.count(S) >= 1, steps                         # (b) one never stops
    for b, n in enumerate(steps):                              # (c) 1e-3 clear of the threshold up to the stop
        assert float((p[b, 1:n] - thr).abs().min()) >= 1e-3
    ref = C.reference("stop_probe", "fp64", thr)
    assert tuple(int(v) for v in ref["y_lengths"]) == tuple(2 * n for n in steps)
    assert ref["decoder_outputs"].shape[1] == 2 * S
    for b, n in enumerate(steps):
        for k, f in (("decoder_outputs", 2), ("model_outputs", 2), ("alignments", 1), ("stop_tokens", 1)):
            assert float(ref[k][b, f * n:].abs().max() if n < S else 0.0) == 0.0
        assert float(ref["decoder_outputs"][b, : 2 * n].abs().min()) > 0.0


def test_edge_cases_cover_the_tile_edges():
    assert C.EDGE_T == (1, 7, 31, 33, 131, 257) and C.edge_lengths(131) == (131, 128, 129, 1)
    assert C.edge_lengths(257) == (257, 128, 129, 1)
    assert C.edge_lengths(7) == (7, 7, 7, 1)
    assert math.isfinite(float(C.reference("edge1")["model_outputs"].abs().max()))
