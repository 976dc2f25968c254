"""torchrun entry point for text-recognition evaluation on MI355X -- same CLI (`--work-dir`), same `test_config.py` contract
and log lines as the reference tools/test_text_recognition_model.py:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.test_text_recognition_model --work-dir ./

    model: <network>, params: ...
    then per validation set `eval dataset:<names joined with [+]>` and one `key: value` line per entry of its result dict
    (the two per-image times, test_loss, str_acc, not_included_str_percent, final_edit_distance, lcs_precision, lcs_recall)

The reference's flops / macs line needs one input size; the images here are 32 x W with W per batch, so only the parameter count is
logged.  As in the reference the loaders are NOT sharded (every rank evaluates every set; rank 0 logs)."""
import argparse
import functools

from . import entry
from .text_scripts import test_text_recognition_for_all_dataset


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Text Recognition Testing (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get testing config')
    return parser.parse_args()


TASK = entry.TestTask(validate=test_text_recognition_for_all_dataset,
                      eval_loaders=functools.partial(entry.dataset_list_loaders, collater='test_collater'), report=entry.report_datasets,
                      describe=lambda config, model: f'params: {sum(p.numel() for p in model.parameters())}')


def main():
    entry.test(parse_args, TASK)


if __name__ == '__main__':
    main()
