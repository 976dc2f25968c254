"""torchrun entry point for universal-segmentation evaluation on a semantic-segmentation dataset, on MI355X -- same CLI (`--work-dir`), same `test_config.py` contract
and log lines as the reference tools/test_universal_segmentation_model_for_semantic_segmentation_dataset.py:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.test_universal_segmentation_model_for_semantic_segmentation_dataset --work-dir ./

    model: <network>, flops: ..., macs: ..., params: ...
    then one `key: value` line per entry of the result dict (the two per-image times, exist_num_class,
    mean_precision, mean_recall, mean_iou, mean_dice)

As in the reference the test loader is NOT sharded (every rank evaluates the whole set; rank 0 logs)."""
import argparse

from . import entry
from .universal_segmentation_scripts import test_semantic_segmentation_dataset


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Universal Segmentation Testing (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get testing config')
    return parser.parse_args()


TASK = entry.TestTask(validate=test_semantic_segmentation_dataset, eval_loaders=entry.whole_test_loader, report=entry.report_result,
                      extra_args=lambda config: (config.decoder, ))


def main():
    entry.test(parse_args, TASK)


if __name__ == '__main__':
    main()
