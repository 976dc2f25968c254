"""torchrun entry point for detection evaluation on MI355X -- same CLI (`--work-dir`), same `test_config.py` contract and log lines as
the reference tools/test_detection_model.py (:29-98):

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.test_detection_model --work-dir ./

    model: <network>, flops: ..., macs: ..., params: ...
    eval type: COCO | VOC, then one `key: value` line per entry of the result dict

As in the reference the test loader is NOT sharded (every rank decodes the whole set; rank 0 logs).  COCO-style numbers come from
tools/cocoeval_numpy.py (pycocotools is not in the image), VOC-style ones from the per-class AP of tools/scripts.py."""
import argparse

from . import entry
from .scripts import test_detection


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Detection Testing (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get testing config')
    return parser.parse_args()


TASK = entry.TestTask(validate=test_detection, eval_loaders=entry.whole_test_loader,
                      report=lambda result_dict, config, info: entry.log_block(info, f'eval type: {config.eval_type}', result_dict),
                      extra_args=lambda config: (config.test_criterion.cuda(), config.decoder))


def main():
    entry.test(parse_args, TASK)


if __name__ == '__main__':
    main()
