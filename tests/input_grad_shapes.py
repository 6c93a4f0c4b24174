"""The kernel constants the input-gradient tests place their shapes by, restated ONCE (``tests/test_input_grad.py`` reads them back
from the sources, ``tests/test_input_grad_gpu.py`` builds its cases from them).

``k_input_grad_v`` (``csrc/dmpnn_inputgrad.hip``): a workgroup per ``FUSED_TILE`` atoms; the operand row ``[GO || S]`` passes through
LDS in chunks of ``FUSED_KCHUNK`` columns of ``GO``, then of ``S``; at most ``FUSED_MAX_DV`` output columns — the dispatch rule
``input_grad_v_fused`` sends a wider ``d_v`` (or rows that are not whole 16-byte quads) to the composed form: ``k_src_sum``, then the
row kernels, whose tile is ``ROW_TILE`` rows."""
FUSED_TILE = 16
FUSED_KCHUNK = 256
FUSED_MAX_DV = 256
ROW_TILE = 48
