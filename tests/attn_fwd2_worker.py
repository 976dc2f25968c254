"""Child process of tests/test_gpu_attn_f64.py::test_fwd2_children.  SAICV_SA_FWD2 is read once per process (a function-local
static of sa_launch, csrc/attn_stream.hip), so the forward kernels only its values 0 and 2 reach need a process of their own:
    python attn_fwd2_worker.py 0 | 2        (the parent also puts the value into the environment)
Runs the bf16 forward rows of attn_common's table against the float64 reference, prints one `CASE` line per case and exits with
status 1 on the first miss."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(value):
    os.environ['SAICV_SA_FWD2'] = value         # before the library's first launch
    import torch
    import attn_common as A
    dt = torch.bfloat16
    for case in A.STREAM_CASES:
        if not A.fwd2_eligible(case):
            continue
        x = A.rounded(A.build_inputs(case), dt)
        got, bad, seed = A.run_stream(case, x, dt, grads=False)
        ref, bnd = A.reference(case, x, seed, grads=False)
        rat = A.ratios(got, ref, bnd, dt)
        form = A.stream_form('bf16', case.D, case.rel_mode, False, case.bias is not None, 0, int(value))
        print(f'CASE {case.id} {form} ' + ' '.join(f'{n}/allowed={r / (A.MARGIN * A.CONSTANTS[dt][n]):.3f}' for n, r in rat.items()), flush=True)
        miss = A.misses(rat, dt)
        if bad or miss:
            print(f'MISS {case.id}: {bad} {miss}', flush=True)
            return 1
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1]))
