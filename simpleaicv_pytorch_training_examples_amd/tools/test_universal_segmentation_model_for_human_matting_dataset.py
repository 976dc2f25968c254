"""torchrun entry point for universal-matting evaluation on the human-matting validation sets, on MI355X -- same CLI (`--work-dir`), same `test_config.py` contract
and log lines as the reference tools/test_universal_segmentation_model_for_human_matting_dataset.py:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.test_universal_segmentation_model_for_human_matting_dataset --work-dir ./

    model: <network>, flops: ..., macs: ..., params: ...
    then per validation set `eval dataset:<names joined with [+]>` and one `key: value` line per entry of its result dict (the
    two per-image times, f_squared_beta_average / _max, mean / max precision and recall, miou_average, miou_max, sad, mae, mse,
    grad, conn)

As in the reference the loaders are NOT sharded (every rank evaluates every set; rank 0 logs)."""
import argparse

from . import entry
from .universal_matting_scripts import validate_human_matting_for_all_dataset


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Universal Matting Testing (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get testing config')
    return parser.parse_args()


TASK = entry.TestTask(validate=validate_human_matting_for_all_dataset, eval_loaders=entry.dataset_list_loaders,
                      report=entry.report_datasets, extra_args=lambda config: (config.decoder, ))


def main():
    entry.test(parse_args, TASK)


if __name__ == '__main__':
    main()
