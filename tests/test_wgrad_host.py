"""MlpParameters on the host: the torch fold against a NumPy float64 fold and against the oracle's own evaluation of the
unfolded net, and autograd through the fold.  No GPU: the module only reads the aircraft's model data."""
import numpy as np
import pytest
import torch

from tests.helpers import make_aircraft
from oracle import Oracle

from aircraft_amd import MlpData, autodiff


def numpy_fold(Ws, bs, act):
    """fold_linear_layers (ac_mlp_model.hpp) in NumPy float64"""
    net = [(np.asarray(W, np.float64), np.asarray(b, np.float64), int(a)) for W, b, a in zip(Ws, bs, act)]
    l = 0
    while l + 1 < len(net):
        if net[l][2]:
            l += 1
            continue
        (Wa, ba, _), (Wb, bb, ab) = net[l], net[l + 1]
        net[l:l + 2] = [(Wb @ Wa, Wb @ ba + bb, ab)]
    return net


def linear_pair_net(seed=3):
    """5-7-9-11-6 with activation-free layers 0 and 1 (two folds in a row) and tanh on layer 2"""
    d = MlpData.synthetic((7, 9, 11), seed=seed)
    d.act = [0, 0, 1, 0]
    return d


NETS = {"shipped": lambda: make_aircraft("nn", normalise=True),
        "tanh_64x3": lambda: make_aircraft("nn", hidden=(64, 64, 64), normalise=True),
        "two_folds": lambda: _with_data(linear_pair_net())}


def _with_data(data):
    ac = make_aircraft("nn", hidden=(8,), normalise=True)
    ac.coefficient_model.data = data
    return ac


@pytest.mark.parametrize("name", list(NETS))
def test_folded_matches_numpy_fold(name):
    ac = NETS[name]()
    d = ac.coefficient_model.data
    params = autodiff.MlpParameters(ac)
    got = params.folded()
    want = numpy_fold(d.weights, d.biases, d.act)
    assert len(got) == len(want)
    if name == "shipped":
        assert [tuple(W.shape) for W, _ in got] == [(32, 5), (6, 32)]  # 5-16-32-6 runs as 5-32-6
    if name == "two_folds":
        assert [tuple(W.shape) for W, _ in got] == [(11, 5), (6, 11)]
    for (W, b), (Wr, br, _) in zip(got, want):
        assert W.dtype == torch.float32 and b.dtype == torch.float32
        # one float32 rounding of the float64 fold
        np.testing.assert_array_equal(W.detach().numpy(), Wr.astype(np.float32))
        np.testing.assert_array_equal(b.detach().numpy(), br.astype(np.float32))
    flat = params.flat().detach().numpy()
    np.testing.assert_array_equal(flat, np.concatenate([np.concatenate([W.astype(np.float32).ravel(), b.astype(np.float32)])
                                                        for W, b, _ in want]))
    # the scalers are buffers, the weights and biases of the UNFOLDED net parameters
    assert {n for n, _ in params.named_buffers()} == {"input_mean", "input_std", "output_mean", "output_std"}
    assert [tuple(p.shape) for p in params.weights] == [w.shape for w in d.weights]
    assert sum(p.numel() for p in params.parameters()) == sum(w.size + b.size for w, b in zip(d.weights, d.biases))


@pytest.mark.parametrize("name", ["shipped", "two_folds"])
def test_oracle_mlp_unfolded_equals_folded(name):
    ac = NETS[name]()
    d = ac.coefficient_model.data
    folded = numpy_fold(d.weights, d.biases, d.act)
    md = d.as_dict()
    md_f = dict(md, weights=[W for W, _, _ in folded], biases=[b for _, b, _ in folded], act=[a for _, _, a in folded])
    rng = np.random.default_rng(0)
    inputs = np.asarray(d.input_mean, np.float64) + np.asarray(d.input_std, np.float64) * rng.normal(size=(200, 5))
    y0, J0 = Oracle(ac.airframe_dict(), "nn", md).mlp(inputs)
    y1, J1 = Oracle(ac.airframe_dict(), "nn", md_f).mlp(inputs)
    assert np.abs(y1 - y0).max() <= 1e-12 * max(1.0, np.abs(y0).max())
    assert np.abs(J1 - J0).max() <= 1e-12 * max(1.0, np.abs(J0).max())


def test_gradient_through_fold_reaches_every_tensor():
    ac = NETS["shipped"]()
    params = autodiff.MlpParameters(ac)
    g = torch.Generator().manual_seed(1)
    flat = params.flat()
    d = torch.randn(flat.shape, generator=g)
    (flat * d).sum().backward()
    for p in params.parameters():
        assert p.grad is not None and p.grad.shape == p.shape and float(p.grad.abs().max()) > 0.0
    # against the closed form for the folded pair (W1 W0, W1 b0 + b1): d/dW0 = W1' D, d/db0 = W1' e, d/dW1 = D W0' + e b0'
    W0, W1 = (w.detach().double() for w in params.weights[:2])
    b0 = params.biases[0].detach().double()
    D = d[: 32 * 5].reshape(32, 5).double()
    e = d[32 * 5: 32 * 6].double()
    torch.testing.assert_close(params.weights[0].grad.double(), W1.T @ D, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(params.biases[0].grad.double(), W1.T @ e, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(params.weights[1].grad.double(), D @ W0.T + torch.outer(e, b0), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(params.biases[1].grad.double(), e, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("model", ["default", "poly"])
def test_analytic_model_is_refused(model):
    with pytest.raises(ValueError, match="MLP surrogate"):
        autodiff.MlpParameters(make_aircraft(model))


# ---- the image of the folded net that ac_set_mlp prepares for k_mlp_wgrad (ac_wgrad.hpp, host part, g++ alone) -----------------
def unpack_fragments(frag, NT, KT):
    """inverse of pack_fragments: [nt][kt][lane][4] -> (16 NT, 16 KT), lane = col + 16 g holding M[16 nt + col][16 kt + 4 g + j]"""
    f = frag.reshape(NT, KT, 4, 16, 4)  # nt, kt, g, col, j
    return f.transpose(0, 3, 1, 2, 4).reshape(16 * NT, 16 * KT)


@pytest.mark.parametrize("name", ["shipped", "tanh_64x3", "ragged_48_80"])
def test_wgrad_image_holds_the_folded_net_and_its_transpose(name, tmp_path):
    import ctypes as C
    import os
    import subprocess

    here = os.path.dirname(os.path.abspath(__file__))
    so = str(tmp_path / "libwgrad_image_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so,
                    os.path.join(here, "host_wgrad", "wgrad_image_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.host_wgrad_image.restype = C.c_long
    ac = NETS[name]() if name in NETS else make_aircraft("nn", hidden=(48, 80), normalise=True)
    d = ac.coefficient_model.data
    n = len(d.weights)
    plan_t = np.dtype([("n_layers", "i4"), ("nin", "i4", 8), ("nout", "i4", 8), ("wf_off", "i4", 8), ("b_off", "i4", 8),
                       ("wt_off", "i4", 8), ("g_off", "i4", 8), ("grad_floats", "i4"), ("image_floats", "i4"), ("act_last", "i4")])
    assert lib.host_wgrad_plan_ints() * 4 == plan_t.itemsize
    plan = np.zeros(1, plan_t)
    image = np.zeros(1 << 20, np.float32)
    wt = C.c_int()
    nf = lib.host_wgrad_image(n, (C.c_int * (n + 1))(*d.widths), (C.c_int * n)(*d.act),
                              (C.c_void_p * n)(*[w.ctypes.data for w in d.weights]),
                              (C.c_void_p * n)(*[b.ctypes.data for b in d.biases]), C.c_void_p(plan.ctypes.data), C.byref(wt),
                              C.c_void_p(image.ctypes.data), C.c_long(image.size))
    p = plan[0]
    assert nf == p["image_floats"] > 0
    folded = numpy_fold(d.weights, d.biases, d.act)
    L, wt = len(folded), wt.value
    assert p["n_layers"] == L and p["act_last"] == 0
    assert wt == {"shipped": 2, "tanh_64x3": 4, "ragged_48_80": 8}[name]
    g = 0
    for l, (W, b, _) in enumerate(folded):
        W32, b32 = W.astype(np.float32), b.astype(np.float32)
        nout, nin = W.shape
        NT, KT = (1 if l == L - 1 else wt), (1 if l == 0 else wt)
        assert (p["nin"][l], p["nout"][l], p["g_off"][l]) == (nin, nout, g)
        g += nout * (nin + 1)
        want = np.zeros((16 * NT, 16 * KT), np.float32)
        want[:nout, :nin] = W32   # padding is exactly zero
        np.testing.assert_array_equal(unpack_fragments(image[p["wf_off"][l]: p["wf_off"][l] + NT * KT * 256], NT, KT), want)
        bias = image[p["b_off"][l]: p["b_off"][l] + 16 * NT]
        np.testing.assert_array_equal(bias[:nout], b32)
        assert not bias[nout:].any()
        if l > 0:   # the transposed block: the A operand of backward-data
            np.testing.assert_array_equal(unpack_fragments(image[p["wt_off"][l]: p["wt_off"][l] + NT * KT * 256], KT, NT), want.T)
    assert p["grad_floats"] == g == autodiff.MlpParameters(ac).flat().numel()
    # activation rows of k_mlp_wgrad fit the 160 KB of a gfx950 workgroup
    assert lib.host_wgrad_lds_bytes(L, wt) == (32 + ((L + 1) * 16 * wt if L > 1 else 0)) * 36 * 4 <= 160 * 1024
