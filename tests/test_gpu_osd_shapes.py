"""The device OSD at its kernel-selection boundaries (tests/osd_shape_codes.py):
every osd_block_kernel / osd_block_cs_kernel instance, osd_kernel<4 | 9 | 17 |
33> (up to 16 waves) and osd_hbm_kernel at its first m and first n, against
the host C++ OSD, the dense NumPy models and the reference's goldens, bit for
bit, on every shot. The models and host results are computed once per process
(osd_shape_codes caches them)."""
import ctypes

import numpy as np
import pytest

import osd_shape_codes as sc

pytestmark = pytest.mark.gpu


def _kernel_name(H, cs):
    from qldpcsim_amd import _lib
    buf = ctypes.create_string_buffer(128)
    _lib.check(_lib.lib.qldpc_osd_kernel_name(_lib.code_for(H, 0).handle, int(cs), buf, 128))
    return buf.value.decode()


def _gpu(H, syn, perms, e0, order=0, lam=None):
    """qldpc_osd_device (lam None) or qldpc_osd_device_cs -> (e_hat, status)."""
    import torch
    from qldpcsim_amd import _lib
    code = _lib.code_for(H, 0)
    pd = torch.as_tensor(np.array(perms, np.int32), device="cuda")
    sd = torch.as_tensor(np.array(syn, np.uint8), device="cuda")
    ed = torch.as_tensor(np.array(e0, np.uint8), device="cuda")
    st = torch.full((len(e0),), -7, dtype=torch.int32, device="cuda")
    if lam is None:
        _lib.check(_lib.lib.qldpc_osd_device(code.handle, len(e0), sd.data_ptr(), pd.data_ptr(), int(order),
                                             ed.data_ptr(), st.data_ptr(), None))
    else:
        _lib.check(_lib.lib.qldpc_osd_device_cs(code.handle, len(e0), sd.data_ptr(), pd.data_ptr(), int(lam),
                                                ed.data_ptr(), st.data_ptr(), None))
    torch.cuda.synchronize()
    return ed.cpu().numpy(), st.cpu().numpy()


def _check_ref(name, what):
    """Orders 0 and 1 of the reference method through whichever kernel the
    options in force select: statuses 0, equal to the host C++ and the model
    on every shot and to the goldens on the golden shots."""
    H, syn, _, e0, perms = sc.shots(name)
    _, m0, m1, _ = sc.ref_model(name)
    g, idx = sc.golden(name), sc.golden_shots(name)
    out = []
    for order, model in ((0, m0), (1, m1)):
        got, st = _gpu(H, syn, perms, e0, order)
        assert got.shape == model.shape == (sc.CASES[name]["k"], H.shape[1])   # no shot left out
        assert np.all(st == 0), (what, order, st)
        np.testing.assert_array_equal(got, sc.host(name, order), err_msg=f"{what}, order {order}: host C++")
        np.testing.assert_array_equal(got, model, err_msg=f"{what}, order {order}: model")
        np.testing.assert_array_equal(got[idx], g[f"ehat{order}"], err_msg=f"{what}, order {order}: reference golden")
        out.append(got)
    return out


@pytest.mark.parametrize("name", sc.IDS)
def test_kernel_names(name, qopt):
    H = sc.matrix(name)
    assert _kernel_name(H, False) == sc.CASES[name]["kernel"]
    if name in sc.BLOCK_IDS:
        assert _kernel_name(H, True) == sc.cs_kernel(name)
        assert sc.cs_kernel(name).startswith("osd_block_cs_kernel<")
        qopt(osd_column=1)
        assert _kernel_name(H, False) == "osd_kernel<%s>" % sc.CASES[name]["kernel"].split("<")[1].split(",")[0]
        qopt(osd_column=0)
    else:
        with pytest.raises(NotImplementedError):
            _kernel_name(H, True)
    if name in sc.HBM_FORCED_IDS:
        qopt(osd_hbm=1)
        assert _kernel_name(H, False) == "osd_hbm_kernel"


def test_every_selectable_instance_is_named():
    # the six block instances (and their CS twins), the four column kernels, the HBM kernel
    names = {sc.CASES[n]["kernel"] for n in sc.IDS} | {sc.cs_kernel(n) for n in sc.BLOCK_IDS}
    want = {f"osd_block{cs}_kernel<{nw}, {sl}, {rt}>" for cs in ("", "_cs") for nw in (4, 9, 17)
            for sl, rt in ((4, 1), (8, 2))} | {"osd_kernel<17>", "osd_kernel<33>", "osd_hbm_kernel"}
    assert names == want


@pytest.mark.parametrize("name", sc.IDS)
def test_reference_method_equals_host_model_and_goldens(name):
    _check_ref(name, sc.CASES[name]["kernel"])


@pytest.mark.parametrize("name", sc.BLOCK_IDS)
def test_column_kernel_alone_equals_the_block_path(name, qopt):
    H, syn, _, e0, perms = sc.shots(name)
    blk = [_gpu(H, syn, perms, e0, order)[0] for order in (0, 1)]
    qopt(osd_column=1)
    col = _check_ref(name, "option osd_column")
    for order in (0, 1):
        np.testing.assert_array_equal(col[order], blk[order], err_msg=f"order {order}")


@pytest.mark.parametrize("name", sc.HBM_FORCED_IDS)
def test_hbm_kernel_equals_the_default_path(name, qopt):
    H, syn, _, e0, perms = sc.shots(name)
    dflt = [_gpu(H, syn, perms, e0, order)[0] for order in (0, 1)]
    qopt(osd_hbm=1)
    hbm = _check_ref(name, "option osd_hbm")
    for order in (0, 1):
        np.testing.assert_array_equal(hbm[order], dflt[order], err_msg=f"order {order}")


@pytest.mark.parametrize("name", sc.BLOCK_IDS)
def test_device_cs_equals_host_and_model(name):
    H, syn, _, e0, perms = sc.shots(name)
    for lam in sc.LAMBDAS:
        got, st = _gpu(H, syn, perms, e0, lam=lam)
        assert got.shape == (sc.CASES[name]["k"], H.shape[1])
        assert np.all(st == 0), (lam, st)
        np.testing.assert_array_equal(got, sc.host_cs(name, lam), err_msg=f"lambda {lam}: host C++")
        np.testing.assert_array_equal(got, sc.cs_model(name, lam)[0], err_msg=f"lambda {lam}: model")


@pytest.mark.parametrize("name", sc.OTHER_IDS)
def test_cs_is_refused_before_any_launch(name):
    import torch
    from qldpcsim_amd import _lib
    H, syn, _, e0, perms = sc.shots(name)
    code = _lib.code_for(H, 0)
    # null device buffers: a refusal that came after the argument checks, let alone a launch, would not be this one
    rc = _lib.lib.qldpc_osd_device_cs(code.handle, len(e0), None, None, 10, None, None, None)
    assert rc == _lib.QLDPC_EUNSUP
    with pytest.raises(NotImplementedError, match="block kernel"):
        _gpu(H, syn[:2], perms[:2], e0[:2], lam=10)
    torch.cuda.synchronize()


def _decode_result(post, e0):
    """A device decode's result with every shot unconverged."""
    import torch
    from qldpcsim_amd import decoders
    k = len(e0)
    return decoders.DecodeResult(torch.as_tensor(np.array(e0), device="cuda"),
                                 torch.zeros(k, dtype=torch.int32, device="cuda"),
                                 torch.as_tensor(np.array(post), device="cuda"),
                                 torch.zeros(k, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("name", ["st3", "st5"])
def test_apply_osd_device_equals_the_goldens(name, osdpol):
    """Through the package, the device reliability order included (n = 693 and
    n = 1211): the golden posteriors, whose order is the committed permutation."""
    import torch
    from qldpcsim_amd import decoders
    osdpol(device_min=1)
    g = sc.golden(name)
    sd = torch.as_tensor(np.array(g["syn"]), device="cuda")
    for order in (0, 1):
        res = _decode_result(g["post"], g["e0"])
        decoders.apply_osd_device(np.array(g["H"]), sd, res, order)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(res.ehat.cpu().numpy(), g[f"ehat{order}"], err_msg=f"order {order}")


def test_apply_osd_device_cs_equals_the_model(osdpol):
    import torch
    from qldpcsim_amd import decoders
    osdpol(device_min=1)
    name, lam = "st3", 10
    H, syn, _, e0, perms = sc.shots(name)
    post = np.stack([sc.order_posteriors(perms[i], e0[i]) for i in range(len(e0))])
    idx = sc.golden_shots(name)
    assert post[idx].tobytes() == sc.golden(name)["post"].tobytes()          # the golden posteriors, every shot
    res = _decode_result(post, e0)
    decoders.apply_osd_device(np.array(H), torch.as_tensor(np.array(syn), device="cuda"), res, lam, method="cs")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(res.ehat.cpu().numpy(), sc.cs_model(name, lam)[0])
