"""Glow-TTS alignment on MI355X: the log-likelihood GEMM (tts_glow_mas_logp), Monotonic Alignment
Search (tts_maximum_path, tts_amd.tts.maximum_path) and GlowTTS.forward / inference_with_MAS.

The search is one fp32 max and one fp32 add per cell in the reference's order, so the device path is
compared with ``mas_ref`` (the reference's loops in numpy float32, vectorised over the tokens of a
column) with torch.equal: no tolerance."""
import math

import numpy as np
import pytest
import torch

from _util import FP32_REL_RMS, WAV_MAX_ABS, assert_close_fp32, goldens, log_error, max_abs, rel_rms
from tts_amd import _native as N
from tts_amd import synthetic
from tts_amd.tts import GlowTTS, maximum_path
from tts_amd.tts.helpers import mas_logp, maximum_path_lengths

pytestmark = pytest.mark.gpu
GTTS = goldens("glow_tts")
# the mel gates of tests/test_glow_tts_gpu.py
MEL_MAX_ABS = 5e-5
MEL_REL_RMS = 5e-6


def mas_ref(v, tx, ty, dtype=np.float32):
    """maximum_path_each (helpers.py / maximum_path.pyx) on one item: v [T_en][T_de] already masked."""
    T_en, T_de = v.shape
    path = np.zeros((T_en, T_de), np.float32)
    if tx < 1 or ty < tx:
        return path
    V = v.astype(dtype).copy()
    NEG = dtype(-1e9)
    xs = np.arange(T_en)
    for y in range(ty):
        lo, hi = max(0, tx + y - ty), min(tx, y + 1)
        x = xs[lo:hi]
        v_cur = np.where(x == y, NEG, V[lo:hi, y - 1])
        v_prev = np.where(x == 0, dtype(0.0) if y == 0 else NEG, V[np.maximum(x - 1, 0), y - 1])
        V[lo:hi, y] = np.maximum(v_cur, v_prev) + V[lo:hi, y]
    index = tx - 1
    for y in range(ty - 1, -1, -1):
        path[index, y] = 1.0
        if index != 0 and (index == y or V[index, y - 1] < V[index - 1, y - 1]):
            index -= 1
    return path


def mas_ref_batch(value, lens, mask=None):
    v = value.numpy() if mask is None else (value * mask).numpy()
    return torch.from_numpy(np.stack([mas_ref(v[b], tx, ty) for b, (tx, ty) in enumerate(lens)]))


def check_path_properties(path, dur, lens):
    for b, (tx, ty) in enumerate(lens):
        p = path[b]
        if tx < 1 or ty < tx:
            assert not p.any() and not dur[b].any()
            continue
        assert torch.equal(p.sum(0)[:ty], torch.ones(ty)), "one token per valid frame"
        assert not p[:, ty:].any() and not p[tx:].any()
        assert ((p == 0) | (p == 1)).all()
        idx = p[:, :ty].argmax(0)
        step = idx[1:] - idx[:-1]
        assert idx[0] == 0 and idx[-1] == tx - 1 and ((step == 0) | (step == 1)).all()
        assert torch.equal(dur[b], p.sum(-1)) and dur[b].sum() == ty


def make_values(kind, B, T_en, T_de, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        return torch.randn(B, T_en, T_de, generator=g)
    return torch.randint(-2, 3, (B, T_en, T_de), generator=g).float()  # exact ties: the strict <


# 64 lanes x {1, 2, 4, 8} tokens per lane; (255, 300): the last lane of the 4-token kernel holds three
# tokens, decision bits in LDS; (257, 1600): one token past 64 x 4, and 50 chunks of 512 words exceed
# the 96 KiB of LDS, so the bits go through the workspace
PATH_CASES = [
    (3, 5, 7, [(5, 7), (5, 5), (1, 7)]),
    (3, 70, 150, [(70, 150), (65, 66), (33, 150)]),
    (2, 130, 300, [(130, 300), (129, 257)]),
    (2, 255, 300, [(255, 300), (254, 255)]),
    (3, 257, 1600, [(257, 1600), (256, 1599), (255, 1537)]),
]
_cache = {}


def path_case(kind, case):
    """(value, reference path) of a case, computed once and shared (never modified)."""
    key = (kind, case[:3])
    if key not in _cache:
        B, T_en, T_de, lens = case
        value = make_values(kind, B, T_en, T_de, seed=T_en * 7 + T_de)
        _cache[key] = (value, mas_ref_batch(value, lens))
    return _cache[key]


def lens_tensors(lens, dev):
    return (torch.tensor([l[0] for l in lens], device=dev), torch.tensor([l[1] for l in lens], device=dev))


@pytest.mark.parametrize("kind", ["normal", "ints"])
@pytest.mark.parametrize("case", PATH_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in PATH_CASES])
def test_path_exact(cuda_device, kind, case):
    B, T_en, T_de, lens = case
    value, ref = path_case(kind, case)
    starts_only = (B * (T_en + 1) * 4 + 255) // 256 * 256  # more: the decision bits are in the workspace
    assert (N.lib().tts_maximum_path_workspace_bytes(B, T_en, T_de) > starts_only) == (T_de == 1600)
    t_x, t_y = lens_tensors(lens, cuda_device)
    path, dur, log_dur = maximum_path_lengths(value.to(cuda_device), t_x, t_y)
    path, dur, log_dur = path.cpu(), dur.cpu(), log_dur.cpu()
    assert torch.equal(path, ref)
    check_path_properties(path, dur, lens)
    assert max_abs(log_dur.numpy(), np.log1p(dur.double().numpy())) <= WAV_MAX_ABS


def test_invalid_items_give_zeros(cuda_device):
    lens = [(6, 9), (6, 4), (0, 5)]
    value = make_values("normal", 3, 6, 9, seed=5)
    t_x, t_y = lens_tensors(lens, cuda_device)
    path, dur, log_dur = maximum_path_lengths(value.to(cuda_device), t_x, t_y)
    assert torch.equal(path.cpu(), mas_ref_batch(value, lens))
    assert path[0].any() and not path[1:].any() and not dur[1:].any() and not log_dur[1:].any()
    check_path_properties(path.cpu(), dur.cpu(), lens)


def test_mask_multiply_and_outside_values(cuda_device):
    B, T_en, T_de = 2, 40, 90
    lens = [(40, 90), (31, 77)]
    value = make_values("normal", B, T_en, T_de, seed=11)
    mask = torch.zeros(B, T_en, T_de)
    for b, (tx, ty) in enumerate(lens):
        mask[b, :tx, :ty] = 1.0
    holes = torch.rand(B, T_en, T_de, generator=torch.Generator().manual_seed(12)) < 0.15
    holes[:, 0, :] = False  # row 0 and column 0 carry the reference's length formula
    holes[:, :, 0] = False
    mask = mask * (~holes).float()
    assert [(int(a), int(c)) for a, c in zip(mask.sum(1)[:, 0], mask.sum(2)[:, 0])] == lens
    ref = mas_ref_batch(value, lens, mask)
    got = maximum_path(value.to(cuda_device), mask.to(cuda_device))
    assert torch.equal(got.cpu(), ref)
    assert not torch.equal(ref, mas_ref_batch(value, lens)), "the holes must matter"
    # no mask: whatever lies outside [0, t_x) x [0, t_y) is never read
    clean = mas_ref_batch(value, lens)
    dirty = value.clone()
    for b, (tx, ty) in enumerate(lens):
        dirty[b, tx:, :] = 1e30
        dirty[b, :, ty:] = 1e30
    t_x, t_y = lens_tensors(lens, cuda_device)
    path, _, _ = maximum_path_lengths(dirty.to(cuda_device), t_x, t_y)
    assert torch.equal(path.cpu(), clean)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_maximum_path_drop_in(cuda_device, dtype):
    case = PATH_CASES[1]
    B, T_en, T_de, lens = case
    value, ref = path_case("normal", case)
    mask = torch.zeros(B, T_en, T_de)
    for b, (tx, ty) in enumerate(lens):
        mask[b, :tx, :ty] = 1.0
    v = value.to(cuda_device)
    got = maximum_path(v.to(dtype) if dtype != torch.float32 else v, mask.to(cuda_device))
    assert got.dtype == dtype and got.device == v.device and got.shape == v.shape
    if dtype == torch.float32:
        assert torch.equal(got.cpu(), ref)
    else:  # the search runs on the fp16 values widened to fp32
        assert torch.equal(got.float().cpu(), mas_ref_batch(value.to(dtype).float(), lens))


# ------------------------------------------------------------------------------------------ logp
def logp_formula(om, ls, z):
    """glow_tts.py:218-228 in the dtype of its inputs."""
    s = torch.exp(-2 * ls)
    l1 = torch.sum(-0.5 * math.log(2 * math.pi) - ls, [1]).unsqueeze(-1)
    l2 = torch.matmul(s.transpose(1, 2), -0.5 * (z ** 2))
    l3 = torch.matmul((om * s).transpose(1, 2), z)
    l4 = torch.sum(-0.5 * (om ** 2) * s, [1]).unsqueeze(-1)
    return l1 + l2 + l3 + l4


def logp_inputs(B, C, T_en, T_de, mean_only):
    g = torch.Generator().manual_seed(C * 1000 + T_en)
    om = torch.randn(B, C, T_en, generator=g)
    ls = torch.zeros(B, C, T_en) if mean_only else 0.3 * torch.randn(B, C, T_en, generator=g)
    z = torch.randn(B, C, T_de, generator=g)
    return om, ls, z


LOGP_CASES = [(2, 80, 37, 150, False), (2, 80, 23, 116, True), (1, 13, 5, 9, False)]
# max|d| of the device against fp64 over max|d| of the fp32 CPU evaluation of the same formula: the
# MFMA accumulates the 2C products of an output in one chain where the CPU GEMM sums blocks, and
# logp2 and logp3 cancel.  Measured on MI355X: 1.49, 2.73 and 1.67 on the three cases (device max|d|
# 7.0e-5, 9.4e-5, 4.3e-6); not under 2 on all of them, so the factor stays 4.
LOGP_MAX_RATIO = 4.0


@pytest.mark.parametrize("B,C,T_en,T_de,mean_only", LOGP_CASES, ids=[f"{c[1]}x{c[2]}x{c[3]}" for c in LOGP_CASES])
def test_logp_accuracy(cuda_device, B, C, T_en, T_de, mean_only):
    om, ls, z = logp_inputs(B, C, T_en, T_de, mean_only)
    ref64 = logp_formula(om.double(), ls.double(), z.double())
    cpu32 = logp_formula(om, ls, z)
    dev = mas_logp(om.to(cuda_device), None if mean_only else ls.to(cuda_device), z.to(cuda_device)).cpu()
    assert dev.shape == (B, T_en, T_de) and torch.isfinite(dev).all()
    ma, rr = max_abs(dev.numpy(), ref64.numpy()), rel_rms(dev.numpy(), ref64.numpy())
    ma32, rr32 = max_abs(cpu32.numpy(), ref64.numpy()), rel_rms(cpu32.numpy(), ref64.numpy())
    log_error(f"glow_mas_logp C={C} T_en={T_en} T_de={T_de} device", ma, rr, LOGP_MAX_RATIO * ma32, FP32_REL_RMS)
    log_error(f"glow_mas_logp C={C} T_en={T_en} T_de={T_de} cpu fp32", ma32, rr32)
    print(f"logp C={C} {T_en}x{T_de}: device max|d| {ma:.3e} rel-RMS {rr:.3e}; cpu fp32 max|d| {ma32:.3e} "
          f"rel-RMS {rr32:.3e}; ratio {ma / ma32:.2f}")
    assert rr <= FP32_REL_RMS
    assert ma <= LOGP_MAX_RATIO * ma32, f"max|d| {ma:.3e} vs {LOGP_MAX_RATIO} x {ma32:.3e}"


def test_path_optimal_against_fp64(cuda_device):
    """The device path is optimal for the device logp, and a path's score moves by at most t_y * eps
    between two matrices eps apart: its fp64 score is within 2 t_y eps of the fp64 optimum."""
    B, C, T_en, T_de, _ = LOGP_CASES[0]
    om, ls, z = logp_inputs(B, C, T_en, T_de, False)
    ref64 = logp_formula(om.double(), ls.double(), z.double()).numpy()
    lens = [(37, 150), (29, 131)]
    t_x, t_y = lens_tensors(lens, cuda_device)
    logp = mas_logp(om.to(cuda_device), ls.to(cuda_device), z.to(cuda_device))
    path, _, _ = maximum_path_lengths(logp, t_x, t_y)
    logp, path = logp.cpu().double().numpy(), path.cpu().double().numpy()
    for b, (tx, ty) in enumerate(lens):
        best = mas_ref(ref64[b], tx, ty, dtype=np.float64).astype(np.float64)
        s_ref, s_dev = float((ref64[b] * best).sum()), float((ref64[b] * path[b]).sum())
        eps = float(np.abs(logp[b, :tx, :ty] - ref64[b, :tx, :ty]).max())
        slack = 1e-9 * abs(s_ref)
        print(f"item {b}: S64(ref) {s_ref:.6f} S64(dev) {s_dev:.6f} gap {s_ref - s_dev:.3e} bound {2 * ty * eps:.3e}")
        assert -slack <= s_ref - s_dev <= 2 * ty * eps + slack


# ------------------------------------------------------------------------------------------ GlowTTS
def build_glow_tts(meta, device, decoder_math_mode="fp32", **speaker):
    """as tests/test_glow_tts_gpu.py builds it"""
    ecfg, dcfg = meta["encoder"], meta["decoder"]
    c_in = ecfg.get("c_in_channels", 0)
    if c_in and not speaker:
        speaker = dict(use_d_vector_file=True, d_vector_dim=c_in)
    m = GlowTTS(dict(num_chars=ecfg["num_chars"], inference_noise_scale=meta["noise_scale"],
                     length_scale=meta["length_scale"], **speaker), decoder_math_mode=decoder_math_mode)
    sd = {f"encoder.{k}": v for k, v in synthetic.glow_encoder_state_dict(**ecfg, seed=meta["eseed"]).items()}
    sd.update({f"decoder.{k}": v for k, v in synthetic.glow_decoder_state_dict(**dcfg, seed=meta["dseed"]).items()})
    if hasattr(m, "emb_g"):
        sd["emb_g.weight"] = meta["emb_g"]
    m.load_state_dict(sd)
    m.eval()
    m.store_inverse()
    return m.to(device)


def golden_inputs(arr):
    tok = torch.from_numpy(arr["tokens"])
    lens = torch.from_numpy(arr["lengths"])
    aux = {"d_vectors": torch.from_numpy(arr["d_vectors"])} if "d_vectors" in arr else {}
    return tok, lens, aux


@pytest.mark.parametrize("name,meta,arr", GTTS, ids=[g[0] for g in GTTS])
def test_forward_chained_exact(cuda_device, name, meta, arr):
    dev = cuda_device
    m = build_glow_tts(meta, dev)
    tok, lens, aux = golden_inputs(arr)
    y = torch.from_numpy(arr["mel_ref_fp32"]).transpose(1, 2)
    y_len = torch.from_numpy(arr["y_lengths_ref_fp32"])
    out = m.forward(tok, lens, y, y_len, aux_input=aux)
    B, T_x = tok.shape
    T_y = (y.shape[1] // 2) * 2
    t_y = (y_len // 2) * 2
    assert out["z"].shape == (B, T_y, 80) and out["logdet"].shape == (B,)
    assert out["alignments"].shape == (B, T_y, T_x) and out["total_durations_log"].shape == (B, T_x, 1)
    g = m._speaker_embedding(aux)
    o_mean, o_log_scale, o_dur_log, x_mask = m.encoder(tok, lens, g=g)
    assert torch.equal(out["durations_log"], o_dur_log.transpose(1, 2))
    logp = mas_logp(o_mean, None if m.mean_only else o_log_scale, out["z"].transpose(1, 2)).cpu()
    pairs = [(int(a), int(c)) for a, c in zip(lens, t_y)]
    ref = mas_ref_batch(logp, pairs)
    assert torch.equal(out["alignments"].cpu(), ref.permute(0, 2, 1))
    check_path_properties(ref, ref.sum(-1), pairs)
    om = o_mean.cpu()
    want = torch.zeros(B, 80, T_y)
    for b, (tx, ty) in enumerate(pairs):
        idx = ref[b, :, :ty].argmax(0)
        want[b, :, :ty] = om[b][:, idx]
    assert torch.equal(out["y_mean"].cpu(), want.transpose(1, 2))
    tdl = torch.log(1 + ref.sum(-1).double()) * x_mask.cpu().double()[:, 0]
    assert max_abs(out["total_durations_log"][:, :, 0].cpu().numpy(), tdl.numpy()) <= WAV_MAX_ABS


def round_trip(m, tok, lens, aux, y_len, name, dev):
    """inference with zero noise, then inference_with_MAS on its mel (y_len: the frame counts inference
    arrives at); the alignment must come back exactly for every item whose tokens fill the row (an item
    of odd length loses its last frame)."""
    B, T_x = tok.shape
    inf = m.inference(tok, {"x_lengths": lens, "noise": torch.zeros(B, 80, int(y_len.max())), **aux})
    mel, A = inf["model_outputs"], inf["alignments"].cpu()
    assert A.shape == (B, int(y_len.max()), T_x)
    out = m.inference_with_MAS(tok, lens, y=mel, y_lengths=y_len, aux_input=aux)
    T2 = (mel.shape[1] // 2) * 2
    t_y = (y_len // 2) * 2
    keep = (torch.arange(T2)[None, :] < t_y[:, None]).float()
    full = [b for b in range(B) if int(lens[b]) == T_x]
    assert full
    for b in full:
        assert torch.equal(out["alignments"][b].cpu(), A[b, :T2] * keep[b, :, None]), f"{name} item {b}"
    y_mask = keep.to(dev).unsqueeze(1)
    zm = out["y_mean"].transpose(1, 2) * y_mask
    assert torch.equal(out["model_outputs"], zm.transpose(1, 2))
    g = m._speaker_embedding(aux)
    y_dec, logdet = m.decoder(zm, y_mask, g=g, reverse=True)
    assert (out["logdet"] is None and logdet is None) or torch.equal(out["logdet"], logdet)
    assert torch.equal(out["y"], y_dec.transpose(1, 2))
    for b in full:  # the same z under the same mask as inference decoded
        ty = int(t_y[b])
        assert_close_fp32(out["y"][b, :ty].cpu(), mel[b, :ty].cpu().double(), f"{name} y item {b}", MEL_MAX_ABS,
                          MEL_REL_RMS)


@pytest.mark.parametrize("name,meta,arr", GTTS, ids=[g[0] for g in GTTS])
def test_inference_with_mas_round_trip(cuda_device, name, meta, arr):
    """With zero noise z = y_mean, so the generating path scores 0 in the quadratic term and any other
    path loses at least min_x 0.5 |mean_x - mean_x+1|^2 (asserted >= 1 below; the flow's round-trip
    error is orders of magnitude smaller).

    GlowTTS.inference gives every padded token of a ragged item one frame that no token owns
    (glow_tts.py:351: clamp_min after the mask), so its alignment is no complete monotonic path and
    cannot be what the search returns.  The batch call therefore pins the items whose tokens fill the
    row, and each ragged item is run alone without its padding, where its alignment is complete: every
    item of the goldens is checked exactly."""
    dev = cuda_device
    tok, lens, aux = golden_inputs(arr)
    xm = arr["x_m_ref_fp64"]
    for b, n in enumerate(lens.tolist()):
        if n > 1:
            d = 0.5 * ((xm[b, :, 1:n] - xm[b, :, :n - 1]) ** 2).sum(0)
            assert d.min() >= 1.0, f"{name} item {b}: neighbouring means {d.min():.3f} apart"
    m = build_glow_tts(meta, dev)
    round_trip(m, tok, lens, aux, torch.from_numpy(arr["y_lengths_ref_fp32"]), name, dev)
    odd = 0
    for b, n in enumerate(lens.tolist()):
        if n == tok.shape[1]:
            continue
        frames = int(arr["w_ceil_ref_fp32"][b, 0, :n].sum())
        odd += frames % 2
        aux_b = {k: v[b:b + 1] for k, v in aux.items()}
        round_trip(m, tok[b:b + 1, :n], lens[b:b + 1], aux_b, torch.tensor([frames]), f"{name} item {b} alone", dev)
    assert odd >= 1, "the goldens hold an item of odd length"


def test_forward_trims_to_the_squeeze(cuda_device):
    name, meta, arr = GTTS[0]
    m = build_glow_tts(meta, cuda_device)
    tok, lens, aux = golden_inputs(arr)
    B, T_x = tok.shape
    y = torch.randn(B, 117, 80, generator=torch.Generator().manual_seed(3))
    out = m.forward(tok, lens, y, aux_input=aux)  # y_lengths=None: all frames
    assert out["z"].shape == (B, 116, 80) and out["alignments"].shape == (B, 116, T_x)
    assert torch.equal(out["alignments"].sum(2).cpu(), torch.ones(B, 116))
    y_len = torch.tensor([117, 101, 55][:B] + [117] * max(0, B - 3))
    out = m.forward(tok, lens, y, y_len, aux_input=aux)
    assert out["y_mean"].shape == (B, 116, 80)
    want = (torch.arange(116)[None, :] < (y_len // 2 * 2)[:, None]).float()
    assert torch.equal(out["alignments"].sum(2).cpu(), want)
    dur = torch.expm1(out["total_durations_log"][:, :, 0].double().cpu())
    assert torch.equal(dur.round().sum(1), (y_len // 2 * 2).double())
