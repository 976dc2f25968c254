"""torchrun entry point for classification training on MI355X -- same CLI (`--work-dir`), same
`train_config.py` contract, same log lines and checkpoint schema as the reference
tools/train_classification_model.py (:33-279), launched the same way:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.train_classification_model --work-dir ./

One process per GPU; process group backend "nccl" (= RCCL over xGMI on ROCm).
Checkpoints: checkpoints/latest.pth = {epoch, time, best_acc1, test_loss, lr, model_state_dict
(`module.`-prefixed), [ema_model_state_dict], optimizer_state_dict, scheduler_state_dict};
best weights (unprefixed) -> best.pth -> `{network}-acc{best:.3f}.pth` at the end.
"""
import argparse

from . import entry
from .scripts import test_classification, train_classification


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Classification Training (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get training config and saving log/models')
    return parser.parse_args()


def evaluate(run, config, epoch, info, acc1, test_loss):
    """every epoch, on the sharded test set, in one line"""
    acc1, acc5, test_loss, per_image_load_time, per_image_inference_time = run()
    info(f'eval: epoch: {epoch:0>3d}, acc1: {acc1:.3f}%, acc5: {acc5:.3f}%, test_loss: {test_loss:.4f}, '
         f'per_image_load_time: {per_image_load_time:.3f}ms, per_image_inference_time: '
         f'{per_image_inference_time:.3f}ms')
    return acc1, test_loss


TASK = entry.TrainTask(train=train_classification, best=entry.BEST_ACC1, eval_loaders=entry.sharded_test_loader,
                       validate=test_classification, evaluate=evaluate)


def main():
    entry.train(parse_args, TASK)


if __name__ == '__main__':
    main()
