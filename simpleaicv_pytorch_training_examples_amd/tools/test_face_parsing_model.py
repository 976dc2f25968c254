"""torchrun entry point for face-parsing evaluation on MI355X -- same CLI (`--work-dir`), same `test_config.py` contract
and log lines as the reference tools/test_face_parsing_model.py:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.test_face_parsing_model --work-dir ./

    model: <network>, flops: ..., macs: ..., params: ...
    then per validation set `eval dataset:<names joined with [+]>` and one `key: value` line per entry of its result dict
    (test_loss, the two per-image times, exist_num_class, mean_precision / mean_recall / mean_iou / mean_dice, then
    class_i_precision, class_i_recall, class_i_iou, class_i_dice for every class)

As in the reference the loaders are NOT sharded (every rank evaluates every set; rank 0 logs)."""
import argparse

from . import entry
from .face_parsing_scripts import validate_face_parsing_for_all_dataset


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Face Parsing Testing (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get testing config')
    return parser.parse_args()


TASK = entry.TestTask(validate=validate_face_parsing_for_all_dataset, eval_loaders=entry.dataset_list_loaders,
                      report=entry.report_datasets)


def main():
    entry.test(parse_args, TASK)


if __name__ == '__main__':
    main()
