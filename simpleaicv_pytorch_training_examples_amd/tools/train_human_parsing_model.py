"""torchrun entry point for human-parsing training on MI355X -- same CLI (`--work-dir`), same
`train_config.py` contract, same log lines and checkpoint schema as the reference
tools/train_human_parsing_model.py, launched the same way:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.train_human_parsing_model --work-dir ./

One process per GPU; process group backend "nccl" (= RCCL over xGMI on ROCm).  The evaluation runs at the epochs of
`config.eval_epoch` and at the last one, on every (unsharded) validation set of `config.val_dataset_list` on every rank, as in the
reference; the best model is the one with the highest `config.save_model_metric` (`mean_iou`) of the FIRST set's result dict, and
every `config.save_interval` epochs the weights are also kept as `epoch_{n}.pth`.
Checkpoints: checkpoints/latest.pth = {epoch, time, best_metric, test_loss, lr, model_state_dict
(`module.`-prefixed), [ema_model_state_dict], optimizer_state_dict, scheduler_state_dict};
best weights (unprefixed) -> best.pth -> `{network}-metric{best:.3f}.pth` at the end.
"""
import argparse

from . import entry
from .human_parsing_scripts import train_human_parsing, validate_human_parsing_for_all_dataset


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Human Parsing Training (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get training config and saving log/models')
    return parser.parse_args()


TASK = entry.TrainTask(train=train_human_parsing, best=entry.BEST_METRIC, criterion_dict=True,
                       eval_loaders=entry.dataset_list_loaders, validate=validate_human_parsing_for_all_dataset,
                       evaluate=entry.evaluate_first_dataset, epoch_weights=True)


def main():
    entry.train(parse_args, TASK)


if __name__ == '__main__':
    main()
