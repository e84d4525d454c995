"""The known-entry list kernels (csrc/skf_known.h) on the hardware, every variant launch_srp picks (csrc/skf_stages.inc) and
the 0 / 1 relations kept as lists, held to the host model of one iteration (tests/known_cases.py: the error model behind
every bound, the mask patterns) -- empty rows and columns, exact list lengths around the batch of 64 and the chunk
cut-offs of srp_bf16_v6_kernel, full rows and columns, entries only in the last part, at the last column, on both sides
of every part boundary, heavy-tailed degrees; row and column counts not multiples of 4, 32 or 64."""
import pytest

import known_cases as K

pytestmark = pytest.mark.gpu

N_A, N_B = 459, 453         # 8 parts of 64 rows / columns, the last one a tail of 11 / 5

# rank of the row type -> kernel (launch_srp): the gathered vectors of both passes are c_i wide
VARIANTS = [('f64', 16), ('f64', 32), ('f64', 64), ('f64', 128), ('f64', 20),          # srp_vec_kernel<double, double, 8..64>, any
            ('f32', 32), ('f32', 64), ('f32', 128), ('f32', 256), ('f32', 24),         # srp_vec_kernel<float, float, 8..64>, any
            ('bf16', 64), ('bf16', 128), ('bf16', 256), ('bf16', 512), ('bf16', 20)]   # srp_bf16_kernel<8>, v6<1>, <32> + v6<2>,
                                                                                       # srp_vec_kernel<uint16_t, float, 64>, any


@pytest.mark.parametrize('parts', [1, 2, 4, 8])
@pytest.mark.parametrize('dtype,rank_a', VARIANTS)
def test_known_entry_lists_against_host_model(dtype, rank_a, parts, monkeypatch):
    for pattern in ('edges', 'full', 'heavy'):
        K.list_case(N_A, N_B, rank_a, 16, dtype, parts, pattern, 'GPU %s rank %d parts %d %s' % (dtype, rank_a, parts, pattern),
                    monkeypatch, seed=parts)


@pytest.mark.parametrize('parts', [1, 2, 4, 8])
@pytest.mark.parametrize('rank_a,rank_b', [(64, 128), (256, 64), (128, 256)])
def test_known_ones_lists_against_host_model(rank_a, rank_b, parts, monkeypatch):
    for pattern in ('edges', 'full', 'heavy'):
        K.ones_case(N_A, N_B, rank_a, rank_b, parts, pattern, 'GPU ones %d x %d parts %d %s' % (rank_a, rank_b, parts, pattern),
                    monkeypatch, seed=parts)
