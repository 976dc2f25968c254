"""torchrun entry point for classification evaluation on MI355X -- same CLI (`--work-dir`), same `test_config.py` contract and the
same two log lines as the reference tools/test_classification_model.py (:31-103):

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.test_classification_model --work-dir ./

    model: <network>, flops: ..., macs: ..., params: ...
    acc1: ..%, acc5: ..%, test_loss: .., per_image_load_time: ..ms, per_image_inference_time: ..ms

One process per GPU, DistributedSampler over the test set, the engine's DDP wrapper around the model (evaluation has no gradient
traffic; the wrapper is there for the `module.` state-dict surface and the reduction group test_classification uses)."""
import argparse

from . import entry
from .scripts import test_classification


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Classification Testing (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get testing config')
    return parser.parse_args()


def report(result, config, info):
    acc1, acc5, test_loss, per_image_load_time, per_image_inference_time = result
    info(f'acc1: {acc1:.3f}%, acc5: {acc5:.3f}%, test_loss: {test_loss:.4f}, per_image_load_time: {per_image_load_time:.3f}ms, '
         f'per_image_inference_time: {per_image_inference_time:.3f}ms')


TASK = entry.TestTask(validate=test_classification, eval_loaders=entry.sharded_test_loader, report=report)


def main():
    entry.test(parse_args, TASK)


if __name__ == '__main__':
    main()
