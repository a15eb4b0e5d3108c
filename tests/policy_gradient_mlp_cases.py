"""The instantiation matrix of the MLP gradient kernels (k_pgm_pass1 / k_pgm_pass2 <WIDTH, LAYERS>), shared by
tests/test_policy_gradient_mlp_cpu.py (the references alone) and tests/test_policy_gradient_mlp_gpu.py (the kernels):
nets that together reach all six (padded width, hidden layers) pairs, both activations and both output forms under
every padded width -- the paddings of CASES in tests/test_mlp_policy_gpu.py plus the missing <16, 2>. Nothing here
touches the GPU or the library."""
import table_edges as E

# name -> ((WIDTH, LAYERS) the net has to run as, hidden widths, activation, output rows)
MATRIX = {
    "tanh1_o2": ((16, 1), (1,), "tanh", 2),
    "tanh7x13": ((16, 2), (7, 13), "tanh", 1),
    "relu16x16_o2": ((16, 2), (16, 16), "relu", 2),
    "relu29_o2": ((32, 1), (29,), "relu", 2),
    "tanh17": ((32, 1), (17,), "tanh", 1),
    "tanh29x9": ((32, 2), (29, 9), "tanh", 1),
    "relu7x29_o2": ((32, 2), (7, 29), "relu", 2),
    "relu33": ((64, 1), (33,), "relu", 1),
    "tanh64_o2": ((64, 1), (64,), "tanh", 2),
    "relu40x64": ((64, 2), (40, 64), "relu", 1),
    "tanh64x33_o2": ((64, 2), (64, 33), "tanh", 2),
}
# a net whose ReLU units sit near a kink too often under the default seed gets another one here (the cap of
# test_relu_cases_are_rarely_near_a_kink stays); none needs it
SEEDS = {}


def net_seed(name, hidden):
    """the seed both test files draw a net's parameters with (tests/table_edges.py: net)"""
    return SEEDS.get(name, len(hidden) * 10 + hidden[0])


def net(ct, name, hidden, n_out):
    return E.net(ct, hidden, n_out, seed=net_seed(name, hidden))
