"""Generated-code check of csrc/lstm.hip (no GPU needed: hipcc cross-compiles gfx950 assembly): every form of the two recurrent
kernels keeps its state -- the cell state, dh and dc of up to eight hidden-column slices per wave -- in registers for the whole
walk over T: no scratch memory, and no more than the 256 vector registers a 512-thread workgroup may have."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.timeout(600)
def test_recurrent_kernels_use_no_scratch(tmp_path):
    csrc = os.path.join(ROOT, 'simpleaicv_pytorch_training_examples_amd', 'csrc')
    out = str(tmp_path / 'lstm.s')
    subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-S', '--cuda-device-only',
                    '-o', out, os.path.join(csrc, 'lstm.hip')], check=True, capture_output=True)
    kernels = re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(out).read(), re.S)
    fwd = [n for n, _ in kernels if 'lstm_fwd_kernel' in n]
    bwd = [n for n, _ in kernels if 'lstm_bwd_kernel' in n]
    # forward: bf16 and fp32 x 1, 2, 4, 8 slices per wave; backward: the same with dgates in LDS, + fp32 at 8 slices reading them back
    assert len(fwd) == 8 and len(bwd) == 9 and len(kernels) == 17, [n for n, _ in kernels]
    for name, body in kernels:
        scratch = int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', body).group(1))
        vgprs = int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', body).group(1))
        assert scratch == 0, (name, scratch)
        assert vgprs <= 256, (name, vgprs)
    text = open(out).read()
    assert 'v_mfma_f32_16x16x32_bf16' in text and 'v_mfma_f32_16x16x4_f32' in text
