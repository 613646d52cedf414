"""ASYMMETRIC group-wise weights (--w_groupsize g --w_asym; the solver runs WeightQuantizer.find_params with sym = False on every
column group, reference gptq/gptq_utils.py:263-275 over quant_utils.py:446-509) on the CPU: the unchanged oracle over the levels
q - z against the reference's own GPTQ + ActQuantWrapper.forward (tests/golden/wrapper_wgasym_*.npz,
tools/gen_golden_wgroup_asym.py), what ``_real_parts`` recovers from the fake-quantized weights, and the ``backend()`` lines."""
import functools
import glob
import os

import numpy as np
import torch

import oracle
from golden_inputs import make_w
from test_wgroup_cpu import DT, TOL, load

torch.set_grad_enabled(False)
KEYS = {"W", "group_scales", "group_zeros", "qx", "acc_groups", "y", "meta", "mode"}
ACT_KEY = {"static": "s_x", "dyn": "s_x_rows", "agrp": "s_x_groups"}


def cases(golden_dir):
    return sorted(glob.glob(os.path.join(golden_dir, "wrapper_wgasym_*.npz")))


def parts_of(g, c):
    """(q - z, stored = q - 2^(b-1), d = 2^(b-1) - z) of a golden, in the SOLVER's column order: int8 [N, K_pad] twice, int16 [G, N]."""
    G, half = c["K_pad"] // c["g"], 1 << (c["w_bits"] - 1)
    W = g["W"][:, g["perm"]] if "perm" in g else g["W"]
    z = g["group_zeros"]
    assert np.array_equal(z, np.rint(z)) and z.min() >= 0 and z.max() <= 2 * half - 1
    qmz = np.rint(W.reshape(c["N"], G, c["g"]) / g["group_scales"][:, :, None])
    q = qmz + z[:, :, None]
    assert q.min() >= 0 and q.max() <= 2 * half - 1
    shape = (c["N"], c["K_pad"])
    return qmz.reshape(shape).astype(np.int8), (q - half).reshape(shape).astype(np.int8), (half - z).T.astype(np.int16).copy()


def act_scales(g, c):
    """The oracle's keyword for the golden's activation scales."""
    if c["mode"] == "static":
        return dict(sx0=float(g["s_x"]))
    return dict(sx_rows=g["s_x_rows"]) if c["mode"] == "dyn" else dict(s_xg=g["s_x_groups"])


def wrapper_from_golden(g, c, device):
    """The wrapper as this repository's solver leaves it: the quantizer remembers the last group (as upstream) and keeps every
    group's scale and zero point."""
    from fake_quant import hadamard_utils as hu, quant_utils as qu, utils
    lin = torch.nn.Linear(c["K_pad"], c["N"], bias=c["bias"])
    lin.weight.data = torch.from_numpy(g["W"].copy())
    if c["bias"]:
        lin.bias.data = torch.from_numpy(make_w(c["seed"] + 1, (c["N"],), std=0.1))
    wrap = qu.ActQuantWrapper(lin.to(DT[c["dtc"]]).to(device))
    if c["had"] and torch.device(device).type == "cuda":
        hadK, Kh = hu.get_hadK(c["K_pad"])
        wrap.online_full_had, wrap.had_K, wrap.K = True, hadK, Kh
    if c["K_pad"] != c["K_in"]:
        wrap.register_forward_pre_hook(functools.partial(utils.revise_down_input, new_size=c["K_pad"]))
    wq = qu.WeightQuantizer()
    wq.configure(c["w_bits"], perchannel=True, sym=False, mse=False)
    gs, gz = torch.from_numpy(g["group_scales"].copy()), torch.from_numpy(g["group_zeros"].copy())
    wq.scale, wq.zero = gs[:, -1:].clone(), gz[:, -1:].clone()
    wq.groupsize, wq.group_permuted, wq.group_scales, wq.group_zeros = c["g"], False, gs, gz
    if "perm" in g:
        wq.group_permuted, wq.group_perm = True, torch.from_numpy(g["perm"].copy())
    qu.attach_weight_quantizer(wrap, "module", wq)
    return wrap


def test_fixture_set_is_complete(golden_dir):
    paths = cases(golden_dir)
    assert len(paths) == 6 and sum("wrapper_wgasym_ao_" in p for p in paths) == 1
    seen = set()
    for path in paths:
        g, c = load(path)
        assert KEYS | {ACT_KEY[c["mode"]]} <= set(g.files), path
        assert ("perm" in g.files) == ("wrapper_wgasym_ao_" in path)
        G = c["K_pad"] // c["g"]
        assert g["group_scales"].shape == g["group_zeros"].shape == (c["N"], G) and g["acc_groups"].shape == (c["M"], G, c["N"])
        assert len(np.unique(g["group_zeros"])) > 4, path            # the zero points spread over the grid
        seen.add((c["g"], c["K_pad"], c["dtc"], c["mode"], c["had"], "perm" in g.files))
    assert seen == {(128, 1024, 0, "static", False, False), (128, 1280, 1, "static", True, False), (64, 512, 0, "static", False, False),
                    (128, 1024, 1, "dyn", False, False), (128, 1024, 0, "agrp", False, False), (128, 1024, 0, "static", False, True)}


def test_oracle_over_q_minus_z_equals_the_reference_forward(golden_dir):
    for path in cases(golden_dir):
        g, c = load(path)
        qmz, stored, d = parts_of(g, c)
        np.testing.assert_array_equal(stored.astype(np.int32) + np.repeat(d.T, c["g"], axis=1), qmz, err_msg=path)
        assert np.abs(qmz).max() <= 15
        bias = make_w(c["seed"] + 1, (c["N"],), std=0.1) if c["bias"] else None
        if bias is not None and c["dtc"] == 1:
            bias = torch.from_numpy(bias).half().float().numpy()
        kw = act_scales(g, c)
        y, acc = oracle.gemm_wgroup(g["qx"], qmz, g["group_scales"].T.copy(), c["g"], bias=bias, want_acc=True, **kw)
        np.testing.assert_array_equal(acc, g["acc_groups"], err_msg=path)                 # exact integers inside every group
        # ... and they are the stored levels' accumulators plus offset x activation group sum
        r = g["qx"].astype(np.int64).reshape(c["M"], -1, c["g"]).sum(axis=2)              # [M, G]
        acc_s = np.einsum("mgk,ngk->mgn", g["qx"].astype(np.int64).reshape(c["M"], -1, c["g"]), stored.astype(np.int64).reshape(c["N"], -1, c["g"]))
        np.testing.assert_array_equal(acc_s + r[:, :, None] * d.astype(np.int64)[None, :, :], g["acc_groups"], err_msg=path)
        tol = TOL[c["dtc"]] * float(np.abs(g["y"]).max())
        np.testing.assert_allclose(y, g["y"], rtol=0, atol=tol, err_msg=path)


def test_real_parts_recover_the_references_levels_zero_points_and_offsets(golden_dir):
    for path in cases(golden_dir):
        g, c = load(path)
        _, stored, d = parts_of(g, c)
        wrap = wrapper_from_golden(g, c, "cpu")
        wrap.quantizer.configure(bits=8, sym=True)                   # dynamic per-token: nothing to calibrate on the CPU
        assert wrap.backend() == "W4A8 integer (dynamic, weight groups of %d, asymmetric)" % c["g"], (path, wrap.backend())
        p = wrap._real_parts(torch.device("cpu"))
        np.testing.assert_array_equal(p["levels"].numpy(), stored, err_msg=path)          # q - 2^(b-1)
        tbl, gsz, offs = p["w_groups"]
        assert gsz == c["g"] and offs.dtype == torch.int16 and p["w_shift"] is None
        np.testing.assert_array_equal(offs.numpy(), d, err_msg=path)                      # 2^(b-1) - z
        np.testing.assert_array_equal(tbl.numpy(), g["group_scales"].T, err_msg=path)
        assert (p["col_perm"] is not None) == ("perm" in g.files)
    # a quantizer of another grid is still refused: the grid check includes the zero points
    g, c = load(cases(golden_dir)[-1])
    wrap = wrapper_from_golden(g, c, "cpu")
    wrap.quantizer.configure(bits=8, sym=True)
    wrap.weight_quantizers["module"].group_zeros = wrap.weight_quantizers["module"].group_zeros.roll(1, dims=0) * 0 + 3.0
    try:
        wrap._real_parts(torch.device("cpu"))
    except RuntimeError as e:
        assert "not on the attached quantizer's grid" in str(e)
    else:
        raise AssertionError("foreign zero points went through the grid check")


def test_backend_line_names_the_asymmetric_groups_or_the_reason():
    from fake_quant import quant_utils as qu
    lin = torch.nn.Linear(256, 16)
    wrap = qu.ActQuantWrapper(lin)
    wrap.quantizer.configure(bits=8, sym=True)
    wq = qu.WeightQuantizer()
    wq.configure(4, perchannel=True, sym=False)
    wq.find_params(lin.weight.data)
    qu.attach_weight_quantizer(wrap, "module", wq)
    assert wrap.backend() == "W4A8 integer (dynamic)"                # per-channel --w_asym, as before
    wq.groupsize, wq.group_permuted, wq.group_scales = 128, False, torch.ones(16, 2)
    assert wrap.backend() == "simulated (torch ops): asymmetric weights with --w_groupsize: group zero points not recorded"
    wq.group_zeros = torch.full((16, 2), 7.0)
    assert wrap.backend() == "W4A8 integer (dynamic, weight groups of 128, asymmetric)"
    assert "weight groups of 128, asymmetric" in wrap.extra_repr()
    # the refusals that remain keep their messages
    wq.groupsize, wq.group_scales, wq.group_zeros = 32, torch.ones(16, 8), torch.full((16, 8), 7.0)
    assert "weight group size 32" in wrap.backend()
    wq.groupsize, wq.group_scales, wq.group_zeros = 128, torch.ones(16, 2), torch.full((16, 2), 7.0)
    wrap.quantizer.configure(bits=8, sym=False)
    assert "--w_groupsize with asymmetric or per-tensor dynamic activations" in wrap.backend()
    wrap.quantizer.configure(bits=8, sym=True)
    wrap.quantizer.act_per_tensor = True
    assert "--w_groupsize with asymmetric or per-tensor dynamic activations" in wrap.backend()
    wrap.quantizer.act_per_tensor = False
    wrap.quantizer.configure(bits=8, sym=True, groupsize=64)         # --a_groupsize != --w_groupsize
    assert wrap.backend().startswith("simulated")
    wrap.quantizer.configure(bits=8, sym=False, groupsize=128)       # asymmetric activation groups x weight groups
    assert wrap.backend().startswith("simulated")
    wrap.quantizer.configure(bits=8, sym=True, groupsize=128)        # symmetric activation groups of the same size
    assert wrap.backend() == "W4A8 integer (dynamic, weight groups of 128, asymmetric)"
    wrap.quantizer.configure(bits=8, sym=True)
    wrap.split = True
    wrap.split_weights()
    qu.attach_weight_quantizer(wrap, "L2", wq)
    assert "--w_groupsize with the split column" in wrap.backend()
    wrap.split = False
    # int8 weights: the group's integer sum must stay an exact float
    wq8 = qu.WeightQuantizer()
    wq8.configure(8, perchannel=True, sym=False)
    lin8 = torch.nn.Linear(2048, 8)
    wrap8 = qu.ActQuantWrapper(lin8)
    wrap8.quantizer.configure(bits=8, sym=True)
    wq8.find_params(lin8.weight.data)
    wq8.groupsize, wq8.group_permuted, wq8.group_scales, wq8.group_zeros = 1024, False, torch.ones(8, 2), torch.full((8, 2), 100.0)
    qu.attach_weight_quantizer(wrap8, "module", wq8)
    assert "asymmetric 8-bit weight groups of 1024" in wrap8.backend()
    wq8.groupsize, wq8.group_scales, wq8.group_zeros = 512, torch.ones(8, 4), torch.full((8, 4), 100.0)
    assert wrap8.backend() == "W8A8 integer (dynamic, weight groups of 512, asymmetric)"
    # symmetric groups read as before
    wqs = qu.WeightQuantizer()
    wqs.configure(4, perchannel=True, sym=True)
    wqs.find_params(lin.weight.data)
    wqs.groupsize, wqs.group_permuted, wqs.group_scales = 128, False, torch.ones(16, 2)
    qu.attach_weight_quantizer(wrap, "module", wqs)
    assert wrap.backend() == "W4A8 integer (dynamic, weight groups of 128)"


def test_group_wise_rtn_and_the_solver_record_zero_points_the_wrapper_takes():
    """fake_quant.gptq.rtn.rtn_module(groupsize=g) with sym = False records group_zeros next to group_scales; the wrapper's levels and
    offsets rebuild the fake-quantized weights exactly."""
    from fake_quant import quant_utils as qu
    from fake_quant.gptq.rtn import rtn_module
    torch.manual_seed(5)
    root = torch.nn.Module()
    root.a = torch.nn.Linear(256, 24, bias=False)
    root.a.weight.data += 0.05
    qu.add_actquant(root)
    quantizers = {}
    rtn_module(root, "m", 4, False, False, [], quantizers, groupsize=64)
    qz = quantizers["m.a.module"]
    assert not qz.sym and tuple(qz.group_zeros.shape) == (24, 4) and torch.equal(qz.group_zeros, qz.group_zeros.round())
    root.a.quantizer.configure(bits=8, sym=True)
    assert root.a.backend() == "W4A8 integer (dynamic, weight groups of 64, asymmetric)"
    p = root.a._real_parts(torch.device("cpu"))
    tbl, g, offs = p["w_groups"]
    lv = p["levels"].float().reshape(24, 4, 64) + offs.t().float()[:, :, None]
    assert torch.equal((lv * tbl.t()[:, :, None]).reshape(24, 256), root.a.module.weight.data)
