"""What the k-chunked rank pass's tests share (tests/test_rank_many_wide_gpu.py on the GPU, tests/test_rank_wide_plan_cpu.py
without one): the parity cases against the oracle and their inputs, so that the chain-model bound is computed on the very
inputs the GPU test ranks."""
from oracle import oracle

PARITY_N = 1999
PARITY_NQ = (19, 300)
PARITY_WIDTHS = [("bf16", 2304), ("bf16", 2560), ("bf16", 8192), ("f32", 1280), ("f32", 4096)]
PARITY_METRIC = "cos"


def parity_inputs(dtype, d, nq):
    """(queries, corpus) as given to the library, and (prepared queries, prepared corpus): what it stores."""
    q, c = oracle.inputs(PARITY_N, nq, d, 100 + d + nq, PARITY_METRIC)
    qp, cp = oracle.prepared_inputs(q, c, PARITY_METRIC, dtype)
    return q, c, qp, cp
