"""torchrun entry point for semantic-segmentation training on MI355X -- same CLI (`--work-dir`), same
`train_config.py` contract, same log lines and checkpoint schema as the reference
tools/train_semantic_segmentation_model.py, launched the same way:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.train_semantic_segmentation_model --work-dir ./

One process per GPU; process group backend "nccl" (= RCCL over xGMI on ROCm).  The evaluation runs at the epochs of
`config.eval_epoch` and at the last one, on the whole (unsharded) test set on every rank, as in the reference; the best model is
the one with the highest `config.save_model_metric` (`mean_iou`) of its result dict.
Checkpoints: checkpoints/latest.pth = {epoch, time, best_metric, test_loss, lr, model_state_dict
(`module.`-prefixed), [ema_model_state_dict], optimizer_state_dict, scheduler_state_dict};
best weights (unprefixed) -> best.pth -> `{network}-metric{best:.3f}.pth` at the end.
"""
import argparse

from . import entry
from .scripts import test_semantic_segmentation, train_semantic_segmentation


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Semantic Segmentation Training (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get training config and saving log/models')
    return parser.parse_args()


def evaluate(run, config, epoch, info, metric, test_loss):
    """at config.eval_epoch and the last epoch: the metric and test_loss come out of the flat result dict"""
    if entry.eval_due(epoch, config):
        result_dict = run()
        for key, value in result_dict.items():
            if key == config.save_model_metric:
                metric = value
            elif key == 'test_loss':
                test_loss = value
        entry.log_block(info, f'eval: epoch: {epoch:0>3d}', result_dict)
    return metric, test_loss


TASK = entry.TrainTask(train=train_semantic_segmentation, best=entry.BEST_METRIC_PERCENT, criterion_dict=True,
                       eval_loaders=entry.whole_test_loader, validate=test_semantic_segmentation, evaluate=evaluate)


def main():
    entry.train(parse_args, TASK)


if __name__ == '__main__':
    main()
