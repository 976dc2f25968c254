"""torchrun entry point for semantic-segmentation evaluation on MI355X -- same CLI (`--work-dir`), same `test_config.py` contract
and log lines as the reference tools/test_semantic_segmentation_model.py:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.test_semantic_segmentation_model --work-dir ./

    model: <network>, flops: ..., macs: ..., params: ...
    then one `key: value` line per entry of the result dict (test_loss, the two per-image times, exist_num_class,
    mean_precision, mean_recall, mean_iou, mean_dice)

As in the reference the test loader is NOT sharded (every rank evaluates the whole set; rank 0 logs)."""
import argparse

from . import entry
from .scripts import test_semantic_segmentation


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Semantic Segmentation Testing (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get testing config')
    return parser.parse_args()


TASK = entry.TestTask(validate=test_semantic_segmentation, eval_loaders=entry.whole_test_loader, report=entry.report_result)


def main():
    entry.test(parse_args, TASK)


if __name__ == '__main__':
    main()
