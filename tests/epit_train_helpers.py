"""Helper of tests/test_gpu_epit_train.py (no tests here): the reference graph of EPIT in fp64 with the HIP path's ReLU / LeakyReLU decisions.

The graph and the forced-decision machinery live in tests/helpers.py (epit_layers_fp64, epit_hip_masks, epit_forced_fp64_grads), beside those
of the other three models; tests/test_epit_reference.py pins the graph on the numpy oracle and on oracle.lfsr_torch_port.epit_forward."""
from tests.helpers import epit_forced_fp64_grads, epit_hip_masks  # noqa: F401
