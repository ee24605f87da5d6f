"""The bounds of test_ops_parity_gpu.test_stage_regularisers_element_by_element_against_float64 without a GPU: the term chain in
fp32 torch on the host stays under half of them on every case, and a chain that loses ONE term -- an adjacency entry, a face --
is outside them."""
import pytest

from helpers import stage_regularisers_chain
from test_ops_parity_gpu import STAGE_REG_CASES, stage_regulariser_bounds, stage_regulariser_case, stage_regulariser_outputs_close


@pytest.mark.parametrize("case", STAGE_REG_CASES)
def test_fp32_host_chain_is_inside_the_bounds_and_a_lost_term_outside(case):
    prev, cur, faces, adj_orig, weights = stage_regulariser_case(case)
    gout = 0.7
    exact, mass, floor, coef, rtol, corners = stage_regulariser_bounds(prev, cur, faces, adj_orig, weights, gout)
    keys = ("lapd", "grad_cur") + (("grad_prev",) if prev.dim() == 3 else ())
    numpy = lambda out: {k: out[k].numpy() for k in keys}
    host = stage_regularisers_chain(prev, cur, adj_orig, faces, *coef, gout)
    stage_regulariser_outputs_close(numpy(host), exact, mass, floor, rtol, case + " (fp32 on the host)", 0.5)
    assert abs(float(host["value"]) - float(exact["value"])) <= 1e-6 * abs(float(exact["value"]))
    # the vertex with the smallest gradient loses its last neighbour
    v = int(exact["grad_cur"].abs().sum(dim=(0, 2)).argmin())
    j = int(adj_orig[v].nonzero().flatten()[adj_orig[v].nonzero().flatten() != v][-1])
    lost = adj_orig.clone()
    lost[v, j] = 0.0
    with pytest.raises(AssertionError):
        stage_regulariser_outputs_close(numpy(stage_regularisers_chain(prev, cur, lost, faces, *coef, gout)), exact, mass, floor, rtol, case)
    if coef[2] != 0.0:          # the last face is not gathered
        with pytest.raises(AssertionError):
            stage_regulariser_outputs_close(numpy(stage_regularisers_chain(prev, cur, adj_orig, faces[:-1], *coef, gout)), exact, mass,
                                            floor, rtol, case)
