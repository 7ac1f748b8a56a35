"""CPU: what the ngf-288 UCF-101 widths (288 / 576 / 864 / 1152, concats up to 2304 channels) rest on.

  * The oracle restatement (oracle/unet_ref.py) against the REAL reference at these widths: tests/golden/w288_forward.pt
    (tools/gen_w288_golden.py; the nets are tests/w288_cases.py's), under the gate tests/test_oracle_golden.py applies to forward fixtures --
    eps within 1e-4 of its maximum, module taps rtol 1e-4 / atol 2e-5.  tests/test_gpu_w288.py leans on the oracle for its sampler case.
  * The per-part GroupNorm coefficient table of the Winograd kernels (tests/test_wide_conv_cpu.py's walk, imported) for the layers a split
    of four or more parts now takes: CinP = 2064 .. 2304, P in (4, 8).
  * The admission rule with the second constant: Cin <= (P >= 4 ? WINO_MAX_CIN_K4 = 2304 : WINO_MAX_CIN = 2048), the rest as before.
"""
import os

import numpy as np
import pytest
import torch

from oracle import sampler_ref, synth, unet_ref
from tests import test_wide_conv_cpu as T
from tests import w288_cases as W
from tests import wino_rule

WINO_MAX_CIN_K4 = wino_rule.WINO_MAX_CIN_K4
CK = T.CK


def admitted(Cin, CinP, P):
    """The bf16x3 family at 8 x 8 (the fp16 kernels, either piece count: the same, 4 parts at most; conv_wino.cpp: 2 parts at most)."""
    return wino_rule.admits("WINO3", Cin, CinP, P, plane=8)


def admitted_parent(Cin, CinP, P):
    """The rule before the second constant, as the commit before this file's wrote it: the historical comparison."""
    nch = CinP // CK
    return (Cin <= T.WINO_MAX_CIN and CinP % CK == 0 and CinP // max(P, 1) <= T.WINO_TABLE_CH
            and (P < 2 or (P in (2, 4, 8) and nch % P == 0 and nch >= 2 * P)))


# ------------------------------------------------------------------------------------------------ the oracle at this width
@pytest.fixture(scope="module")
def fixture(golden_dir):
    return W.load(golden_dir)


@pytest.mark.parametrize("case", W.CASES)
def test_oracle_forward_matches_reference_at_ngf_288(fixture, case):
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    g = fixture[case]
    config = W.make_config(case)
    sd = synth.make_state_dict(config, seed=g["seed"])
    x, cond = synth.make_inputs(config, g["batch"], seed=0)
    assert torch.equal(x, g["x"]) and torch.equal(cond, g["cond"])          # the stored inputs are synth's
    taps = {}
    with torch.no_grad():
        eps = unet_ref.unet_forward(sd, config, g["x"], g["t"], g["cond"], taps=taps, cond_mask=g.get("mask"))
    ref = g["eps"]
    assert eps.shape == ref.shape
    err = (eps - ref).abs().max().item()
    print(f"{case}: |eps - reference| {err:.3e} of max {ref.abs().max().item():.3f}")
    assert err <= 1e-4 * ref.abs().max().item()
    up = g["up_block"]
    assert up == W.first_up_block(config) and list(taps[up].shape) == [g["batch"], 1152, 8, 8] and list(taps[1].shape) == [g["batch"], 1152]
    torch.testing.assert_close(taps[1], g["tap_temb"], rtol=1e-4, atol=2e-5, msg="module 1 (temb)")
    torch.testing.assert_close(taps[up].reshape(-1)[::W.TAP_STRIDE], g["tap_up"], rtol=1e-4, atol=2e-5, msg=f"module {up} (first up block)")
    assert abs(taps[up].abs().max().item() - g["tap_up_scale"]) <= 1e-4 * g["tap_up_scale"]


def test_oracle_sampler_matches_reference_at_ngf_288(fixture):
    """DDPM, 5 steps + denoise with injected noise: what tests/test_gpu_w288.py holds the device sampler to."""
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    g = fixture["plain"]
    config = W.make_config("plain")
    net = unet_ref.OracleScoreNet(config, synth.make_state_dict(config, seed=g["seed"]))
    noise = synth.make_noise(config, g["batch"], 6, seed=2)
    k = [0]

    def fn(i, like):
        k[0] += 1
        return noise[k[0] - 1]
    out = sampler_ref.sample(g["x"].clone(), net, cond=g["cond"], kind="ddpm", final_only=True, denoise=True, subsample_steps=5,
                             clip_before=True, noise_fn=fn)
    assert k[0] == g["sampler_n_noise"] and out.shape == g["sampler_ddpm5"].shape
    assert (out - g["sampler_ddpm5"]).abs().max().item() <= 1e-4


# ------------------------------------------------------------------------------------------------ the table, 2049 .. 2304 channels
def test_every_family_takes_the_second_constant_where_it_has_four_parts():
    assert wino_rule.header_constants()["WINO_MAX_CIN_K4"] == 2304 == WINO_MAX_CIN_K4 and T.WINO_MAX_CIN == 2048
    for plane in (8, 16):
        # the families with a 4-way split (the fp16 kernels: both piece counts) take the new bound from 4 parts on
        for fam in ("WINO3", "WINO2H", "WINO1H"):
            assert wino_rule.admits(fam, 2304, parts=4, plane=plane) and not wino_rule.admits(fam, 2320, parts=4, plane=plane), (fam, plane)
            assert not wino_rule.admits(fam, 2304, parts=2, plane=plane) and not wino_rule.admits(fam, 2304, parts=1, plane=plane), (fam, plane)
        assert wino_rule.admits("WINO3", 2304, parts=8, plane=plane) and not wino_rule.admits("WINO2H", 2304, parts=8, plane=plane)
        # conv_wino.cpp splits two ways only: its bound stays WINO_MAX_CIN, whatever ksplit says
        for ksplit in (0, 2, 4, 8):
            assert not wino_rule.admits("WINO", 2304, parts=wino_rule.kernel_parts("WINO", ksplit), plane=plane)
        assert wino_rule.admits("WINO", 2048, parts=2, plane=plane)
    # the persistent kernel and the SPADE-fused loader stay at WINO_TABLE_CH
    for parts in (1, 2, 4, 8):
        assert wino_rule.admits("WINO3P", 1024, parts=parts, plane=16) and not wino_rule.admits("WINO3P", 1152, parts=parts, plane=16)
    assert wino_rule.admits("WINO", 1024, plane=16, spade=True) and not wino_rule.admits("WINO", 1040, plane=16, spade=True)
    assert wino_rule.admits("WINO", 1040, plane=16) and not wino_rule.admits("WINO3", 512, plane=16, spade=True)


def test_the_rule_with_the_second_constant():
    assert admitted(2304, 2304, 4) and admitted(2304, 2304, 8)                  # 144 chunks: 36 / 18 per part
    assert not admitted(2304, 2304, 1) and not admitted(2304, 2304, 2)          # one part of 2304 / 1152 channels: more than the table
    assert not any(admitted(2320, 2320, P) for P in (1, 2, 4, 8))
    assert not any(admitted(2305, 2320, P) for P in (1, 2, 4, 8))
    assert not admitted(2160, 2160, 4) and not admitted(2160, 2160, 8)          # 135 chunks
    assert admitted(2290, 2304, 4) and admitted(2176, 2176, 8) and admitted(2176, 2176, 4)          # 136 chunks
    assert not admitted(2064, 2064, 2) and not admitted(2064, 2064, 4)          # 129 chunks
    assert admitted(2112, 2112, 4) and not admitted(2112, 2112, 8)              # 132 chunks
    # up to 2048 channels the rule is the parent's, case by case
    for CinP in range(CK, 2048 + 1, CK):
        for Cin in (CinP, CinP - 7):
            for P in (1, 2, 4, 8):
                assert admitted(Cin, CinP, P) == admitted_parent(Cin, CinP, P), (Cin, CinP, P)
    # and the 2-way split never takes more than WINO_MAX_CIN by the table rule alone
    assert all(not admitted(c, c, 2) for c in range(2064, 2400, CK))


def test_every_layer_of_2049_to_2304_channels_parks_and_reads_its_own_channels():
    cases = seam_inside = seam_on_boundary = 0
    for CinP in range(2064, 2304 + 1, CK):
        nch = CinP // CK
        for Cin in sorted({CinP, CinP - 7, CinP - 15}):
            for P in (4, 8):
                if not admitted(Cin, CinP, P):
                    assert nch % P != 0, (Cin, CinP, P)               # the only reason left in this range
                    continue
                for g8 in (False, True):
                    T._check_tables(Cin, CinP, P, g8)
                    cases += 1
                pp = [T.part_range(nch, P, kh) for kh in range(P)]
                assert pp[0][0] == 0 and pp[-1][1] == nch and all(pp[i][1] == pp[i + 1][0] for i in range(P - 1))
                assert all(e - b == nch // P >= 2 for b, e in pp)
                lo = np.arange(nch) * CK
                lo = lo[lo < Cin]
                last = np.minimum(lo + CK, Cin) - 1
                for C0 in [Cin] + list(range(CK, Cin, CK)):           # the concat seam on a chunk boundary: one source per chunk
                    src = np.array([T.chunk_source(int(c), Cin, C0) for c in lo // CK], dtype=bool)
                    assert ((lo >= C0) == src).all() and ((last >= C0) == src).all(), (Cin, C0)
                    if C0 < Cin:
                        if any(b * CK < C0 < e * CK for b, e in pp):
                            seam_inside += 1
                        else:
                            seam_on_boundary += 1
    print(f"{cases} (Cin, CinP, parts, G8) table walks above 2048 channels; seams inside a part {seam_inside}, on a part boundary {seam_on_boundary}")
    # 129 .. 144 chunks: four counts divide by 4 (132, 136, 140, 144), two by 8 (136, 144); three Cin each, with and without G8
    assert cases == (4 + 2) * 3 * 2 and seam_inside > 100 and seam_on_boundary > 10
    # the cases tests/test_gpu_w288.py forces
    for Cin, CinP, P in ((2304, 2304, 4), (2304, 2304, 8), (2176, 2176, 8), (2290, 2304, 4)):
        assert admitted(Cin, CinP, P)


def test_lds_sizes_at_576_and_288_channels_per_part():
    for g8 in (False, True):
        for pc in (576, 288):
            sizes = {fn.__name__: fn(pc, g8) for fn in (T.lds_wino3, T.lds_wino2h, T.lds_wino1h, T.lds_wino)}
            assert all(v <= T.LDS_MAX for v in sizes.values()), (pc, g8, sizes)
            # a part's table is smaller than the 1024-channel one the parent's widest 2-way launch parks
            assert T.lds_wino3(pc, g8) < T.lds_wino3(1024, g8)
    assert T.lds_wino3(576, True) == (2 * 3 * 16 * 2 * 4 * 32 + 2 * (16 * 10 * 24 + 8) + 4 * 576 + 512) * 4
