"""GPU: the autotuner's table against what the launches then run, under the options that change the candidate rule (conv_tuner.h).

`tiny` and `tiny_spade` at B = 2 under the default options, `f16x2`, `f16x1` and `bf16x3` = 0.  After ONE autotuned forward of a leg:
  * every conv op that ran reports in mcvd_model_op_kernel the id get_tuning names for it: the tuner times a candidate only where the kernel
    takes the layer, so the launch never falls back from what the table says;
  * the table names no id the leg's options forbid (12 / 13 / 14 / 26 without f16x2; 24 / 25 / 27 without f16x1; 10 .. 20, 15, 22, 23 with
    bf16x3 = 0);
  * the same table, installed with autotune = 0 on a fresh net under the same options, gives a bit-identical epsilon;
  * the default leg meets the parity gate 1e-4 * max |eps| against the oracle.
"""
import ctypes as C

import pytest
import torch

from oracle import synth, unet_ref

pytestmark = pytest.mark.gpu

B = 2
OP_CONV = 3                              # model.h: OpKind
LEGS = {"default": {}, "f16x2": {"f16x2": 1}, "f16x1": {"f16x1": 1}, "no_bf16x3": {"bf16x3": 0}}
TWO_PIECE, ONE_PIECE = (12, 13, 14, 26), (24, 25, 27)
NOT_WITHOUT_BF16X3 = tuple(range(10, 21)) + (22, 23)  # the bf16x3 = 0 leg (f16x2 off too): nothing from 10 to 20 -- the three-piece ids and, the
                                                      # option being off, the fp16 ids 12 / 13 / 14 among them -- and neither GEMM form of a 3x3

_CASES = {}


def _case(name):
    """config, weights, inputs and the oracle's epsilon of a net: computed once, shared by the legs, left unchanged."""
    if name not in _CASES:
        config = synth.make_config(name)
        config.device = "cuda:0"
        sd = synth.make_state_dict(config, seed=123)
        x, cond = synth.make_inputs(config, B, seed=0)
        t = torch.tensor([990, 130])
        with torch.no_grad():
            ref = unet_ref.unet_forward(sd, config, x, t, cond)
        _CASES[name] = dict(config=config, sd=sd, x=x.cuda(), cond=cond.cuda(), t=t.cuda(), ref=ref)
    return _CASES[name]


def _net(case, options):
    from mcvd_pytorch_amd.scorenet import HipScoreNet
    net = HipScoreNet(case["config"])
    net.load_state_dict(case["sd"], strict=True)
    for k, v in options.items():
        net.set_option(k, v)
    return net.eval()


def _ran(net):
    """{op index: kernel its last launch ran} of the conv ops of the plan that were launched."""
    from mcvd_pytorch_amd import _lib
    n = _lib.lib.mcvd_model_profile_read(net._model, None, None, None, None, None, 0)
    info, out = (C.c_int * 8)(), {}
    for i in range(n):
        _lib.check(_lib.lib.mcvd_model_op_info(net._model, i, info), "op_info")
        if info[0] == OP_CONV and _lib.lib.mcvd_model_op_kernel(net._model, i) != -1:
            out[i] = _lib.lib.mcvd_model_op_kernel(net._model, i)
    return out


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("name", ["tiny", "tiny_spade"])
def test_the_tuned_table_is_what_runs_and_respects_the_options(name, leg):
    case, options = _case(name), LEGS[leg]
    net = _net(case, options)
    eps = net(case["x"], case["t"], cond=case["cond"]).clone()
    table = net.get_tuning(B)
    ran = _ran(net)
    print(f"{name} / {leg}: (op, table id, cout tile, ran) of the conv ops:", [(i, table[i][0], table[i][1], k) for i, k in ran.items()])
    assert len(ran) >= 10, ran
    # 1. the launch runs what the table names
    fell_back = [(i, table[i], k) for i, k in ran.items() if k != table[i][0]]
    assert not fell_back, f"(op, (table id, cout tile), ran): {fell_back}"
    # 2. nothing the options forbid
    named = {sh for sh, _ in table if sh >= 0}
    forbidden = set()
    if not options.get("f16x2"):
        forbidden |= set(TWO_PIECE)
    if not options.get("f16x1"):
        forbidden |= set(ONE_PIECE)
    if options.get("bf16x3", 1) == 0:
        forbidden |= set(NOT_WITHOUT_BF16X3)
    assert not (named & forbidden), f"the table names {sorted(named & forbidden)} under {options}"
    # 3. the table alone reproduces the forward
    fresh = _net(case, dict(options, autotune=0))
    fresh.set_tuning(B, table)
    again = fresh(case["x"], case["t"], cond=case["cond"]).clone()
    assert _ran(fresh) == ran
    assert torch.equal(again, eps), f"max |difference| {(again - eps).abs().max().item():.3e}"
    # 4. parity of the default arithmetic
    ref = case["ref"]
    err = (eps.cpu() - ref).abs().max().item()
    print(f"{name} / {leg}: |eps - oracle| {err:.3e} of max {ref.abs().max().item():.3f}")
    if leg == "default":
        assert err <= 1e-4 * ref.abs().max().item()
