"""GPU: replacing the backend of a live handle.  tbnn_set_row_weights and tbnn_set_data re-select the kernel family of a handle
(tbnn_api.hip: select_kernels constructs a new Backend and alloc_workspace prepares it): a handle that went through weighted rows,
back to unweighted ones and on to another row count must compute exactly what a fresh handle on the final rows computes -- the
same kernels, the same bits -- on each of the four backends: one-kernel fused, wide, layered, thread-per-row.  No run-time kernel
library is compiled or picked up (TBNN_JIT=0 in this suite, TBNN_REGISTERED=0 here), so the weighted stage of the fused and wide
cases runs on the layered family: the backend object really changes under the handle."""
import numpy as np
import pytest

import tbnn_oracle as o
from test_gpu_layered import scaled_problem

pytestmark = pytest.mark.gpu

N0, N1 = 37, 100            # the first row count is no multiple of the 16-row tile
EPS, L, EPOCHS = 1e-4, 3, 3

# the smallest shapes the family tests reach each backend with: test_gpu_parity.py (c1, wide_t1 under TBNN_MID=0), test_gpu_layered.py
# (mixed_acts under TBNN_TALL=0), TBNN_KERNEL_GENERIC
CASES = {
    "fused": dict(dims=[1, 10, 10, 1], acts=[o.ACT_RELU], prior=o.PRIOR_CAUCHY, lik=o.LIK_GAUSSIAN, env={}, generic=False,
                  name="fast3<", weighted="layered<1,10,10,1,weighted>"),
    "wide": dict(dims=[3, 20, 36, 2], acts=[o.ACT_TANH], prior=o.PRIOR_GAUSSIAN, lik=o.LIK_GAUSSIAN, env={"TBNN_MID": "0"}, generic=False,
                 name="wide<", weighted="layered<3,20,36,2,weighted>"),
    "layered": dict(dims=[4, 8, 8, 1], acts=[o.ACT_RELU, o.ACT_TANH], prior=o.PRIOR_CAUCHY, lik=o.LIK_GAUSSIAN, env={"TBNN_TALL": "0"},
                    generic=False, name="layered<4,8,8,1>", weighted="layered<4,8,8,1,weighted>"),
    "generic": dict(dims=[1, 10, 10, 1], acts=[o.ACT_RELU], prior=o.PRIOR_CAUCHY, lik=o.LIK_GAUSSIAN, env={}, generic=True,
                    name="generic", weighted="generic<weighted>"),
}


def make_chain(native, spec, generic):
    layers = [(l.in_dim, l.out_dim, l.act, l.prior) for l in spec.layers]
    return native.Chain(layers, likelihood=spec.likelihood, fixed_sd=spec.fixed_sd,
                        kernel=native.KERNEL_GENERIC if generic else native.KERNEL_AUTO, jit=False)


def final_calls(ch, X, Y, theta, eta, thetas):
    """what both handles do from the final set_data on: every output, and the kernel name"""
    ch.set_data(X, Y)
    out = {"name": ch.kernel_name}
    out["logp"], out["grad"], out["stat"] = ch.logp_grad(theta, eta)
    out["forward"] = ch.forward(X, theta)
    out["forward_many"] = ch.forward_many(thetas, X=X)
    ch.set_state(theta)
    ch.set_hypers(eta)
    recs = ch.hmc_run(EPS, L, EPOCHS)
    out["records"] = [{k: v for k, v in r.items() if not k.endswith("_us")} for r in recs]      # (all but the timings)
    out["state"] = ch.get_state()
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k, np.abs(a[k] - b[k]).max())
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


@pytest.mark.parametrize("case", list(CASES))
def test_backend_swap_matches_fresh_handle(native, case, monkeypatch):
    c = CASES[case]
    monkeypatch.setenv("TBNN_REGISTERED", "0")       # no kernel library another module registered in this process
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    if len(c["acts"]) > 1:
        spec, X, Y, theta, eta = scaled_problem(c["dims"], N1, c["acts"], c["prior"], c["lik"])
    else:
        spec, X, Y, theta, eta = o.synth_problem(c["dims"], N1, c["acts"][0], c["prior"], c["lik"])
    rng = np.random.default_rng(7)
    w = rng.uniform(0.25, 2.0, N0).astype(np.float32)
    thetas = (theta[None, :] + 0.05 * rng.standard_normal((3, theta.size))).astype(np.float32)

    a = make_chain(native, spec, c["generic"])
    assert a.kernel_name.startswith(c["name"]), a.kernel_name
    name0 = a.kernel_name
    a.set_data(X[:N0], Y[:N0])
    a.set_row_weights(w)
    assert a.kernel_name == c["weighted"], a.kernel_name
    weighted_a = a.logp_grad(theta, eta)
    a.set_row_weights(None)
    assert a.kernel_name == name0, a.kernel_name
    got = final_calls(a, X, Y, theta, eta, thetas)
    a.close()

    b = make_chain(native, spec, c["generic"])
    want = final_calls(b, X, Y, theta, eta, thetas)
    b.close()
    assert want["name"] == name0
    assert_same(got, want, case)

    f = make_chain(native, spec, c["generic"])
    f.set_data(X[:N0], Y[:N0])
    f.set_row_weights(w)
    assert f.kernel_name == c["weighted"], f.kernel_name
    weighted_f = f.logp_grad(theta, eta)
    f.close()
    assert weighted_a[0] == weighted_f[0] and weighted_a[2] == weighted_f[2] and np.array_equal(weighted_a[1], weighted_f[1]), case
