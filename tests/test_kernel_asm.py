"""Generated-code checks of the HIP kernels (no GPU needed: hipcc cross-compiles gfx950 assembly)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


@pytest.mark.timeout(900)
@pytest.mark.parametrize('source', ['elemwise.hip', 'detloss.hip', 'groupnorm.hip'])
def test_streaming_kernels_of_the_late_additions_keep_their_registers(source, tmp_path):
    """The HBM-bound kernels added for the convolutional backbones and the dense detectors (csrc/elemwise.hip, detloss.hip,
    groupnorm.hip) must not spill (no scratch memory) and must leave room for at least four wavefronts per SIMD (<= 128 vector
    registers): their only way to hide HBM latency is occupancy."""
    import re
    import subprocess
    csrc = os.path.join(ROOT, 'simpleaicv_pytorch_training_examples_amd', 'csrc')
    out = str(tmp_path / 'k.s')
    subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-S', '--cuda-device-only',
                    '-o', out, os.path.join(csrc, source)], check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', text, re.S)
    assert len(kernels) >= 6, source
    for name, body in kernels:
        scratch = int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', body).group(1))
        vgprs = int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', body).group(1))
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)


@pytest.mark.timeout(1200)
def test_asm_fragment_reads_of_each_kernel_are_not_touched_before_their_counted_wait():
    """the `ds_read_b128` fragment reads of csrc/igemm.hip and csrc/pwstream.hip are inline asm with `=v` outputs the
    compiler treats as valid at once, released by hand-counted `s_waitcnt lgkmcnt(N)` asm statements.  scripts/check_fragment_regs.py
    replays the LGKM counter over the generated assembly of every kernel: no instruction reads or writes a fragment register while
    its read is outstanding (a copy or spill the register allocator slipped in, or a compiler-generated LDS / scalar-memory
    operation that made a count wrong, would show), and those kernels use no scratch.  The checker itself is checked by mutation:
    a wait count raised by two, and a move inserted behind a read, must both be reported."""
    import re
    import check_fragment_regs as F
    pw = F.assembly('pwstream.hip')
    reports = F.check(pw) + F.check(F.assembly('igemm.hip'))
    assert len([r for r in reports if 'pw_stream_kernel' in r[0]]) == 3           # the nine-tap forms: plain, + statistics, + data-gradient extras
    # + the 26 bf16 forms of igemm_nt1_kernel and the 10 of igemm_tn_dma_kernel
    assert len(reports) == 3 + 26 + 10, len(reports)
    for name, n_reads, n_waits, scratch, bad in reports:
        assert n_reads >= 1 and n_waits >= 1 and scratch == 0 and not bad, (name, n_reads, n_waits, scratch, bad[:3])
    # mutation 1: the first three counted waits release two reads too few
    lines, in_asm, changed = pw.split('\n'), False, 0
    for i, l in enumerate(lines):
        if 'ASMSTART' in l:
            in_asm = True
        elif 'ASMEND' in l:
            in_asm = False
        elif in_asm and 's_waitcnt lgkmcnt(' in l and changed < 3:
            n = int(re.search(r'lgkmcnt\((\d+)\)', l).group(1))
            lines[i] = l.replace(f'lgkmcnt({n})', f'lgkmcnt({n + 2})')
            changed += 1
    assert changed == 3 and sum(len(r[4]) for r in F.check('\n'.join(lines))) > 0
    # mutation 2: a copy of a fragment register right behind its read
    lines, in_asm = pw.split('\n'), False
    for i, l in enumerate(lines):
        if 'ASMSTART' in l:
            in_asm = True
        elif 'ASMEND' in l:
            in_asm = False
        elif in_asm and 'ds_read_b128' in l:
            lines.insert(i + 2, '\tv_mov_b32_e32 v200, v' + re.search(r'v\[(\d+):', l).group(1))
            break
    assert sum(len(r[4]) for r in F.check('\n'.join(lines))) == 1


def _igemm_kernels_expected():
    """The kernels csrc/igemm.hip instantiates (mangled, after the anonymous-namespace prefix): every form a launch can reach, no other."""
    nt1 = 'igemm_nt1_kernelI{}Li{}ELi{}ELi{}ELi{}ELi{}ELb{:d}ELb{:d}ELi{}EEEvNS_8NTParamsE'
    tiles = [(256, 256, 2, 4), (256, 128, 4, 2), (128, 128, 2, 2), (128, 64, 2, 2)]
    names = set()
    for mode in (0, 1):
        for plain in (False, True):
            for tile in tiles:
                wide = tile[:2] == (256, 256)             # bf16 output only: an fp32 output tile would not fit the epilogue LDS
                names.add(nt1.format('DF16b', *tile, mode, False, plain, 4))
                if not wide:
                    if mode == 0:                         # bf16 data with an fp32 output: forward only (no entry point asks a data gradient for it)
                        names.add(nt1.format('DF16b', *tile, mode, True, plain, 4))
                    names.add(nt1.format('f', *tile, mode, True, plain, 4))      # fp32 data always writes fp32
        for tile in tiles[:2]:                            # 128-byte K slices: pointwise bf16, 256-row tiles
            names.add(nt1.format('DF16b', *tile, mode, False, True, 8))
    tn = [(64, 64, 2, 2), (64, 128, 2, 2), (128, 64, 2, 2), (128, 128, 2, 2), (256, 256, 2, 4)]
    for g in tn:
        for t in ('DF16b', 'f'):
            names.add('igemm_tn_kernelI{}Li{}ELi{}ELi{}ELi{}EEEvNS_8TNParamsE'.format(t, *g))
        for plain in (False, True):
            names.add('igemm_tn_dma_kernelILi{}ELi{}ELi{}ELi{}ELb{:d}EEEvNS_8TNParamsE'.format(*g, plain))
    return names


@pytest.mark.timeout(1200)
def test_igemm_instantiates_exactly_the_launchable_kernels():
    """38 igemm_nt1_kernel forms (no fp32 data with a bf16 output, no fp32 output on the 256 x 256 tile, no fp32 output of a bf16
    data gradient), 10 igemm_tn_kernel, 10 igemm_tn_dma_kernel: a form the dispatch cannot reach is not compiled
    (tests/test_igemm_plan_host.py shows that each of them IS reached)."""
    import re
    import check_fragment_regs as F
    found = re.findall(r'^\s*\.amdhsa_kernel _ZN12_GLOBAL__N_1\d+(\S+)$', F.assembly('igemm.hip'), re.M)
    expected = _igemm_kernels_expected()
    assert len(expected) == 58 and len([n for n in expected if n.startswith('igemm_nt1_kernel')]) == 38
    assert len(found) == len(set(found))
    assert set(found) == expected, (sorted(set(found) - expected), sorted(expected - set(found)))
