"""torchrun entry point for text-recognition training on MI355X -- same CLI (`--work-dir`), same
`train_config.py` contract, same log lines and checkpoint schema as the reference
tools/train_text_recognition_model.py, launched the same way:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.train_text_recognition_model --work-dir ./

One process per GPU; process group backend "nccl" (= RCCL over xGMI on ROCm).  The evaluation runs at the epochs of
`config.eval_epoch` and at the last one, on every (unsharded) validation set of `config.val_dataset_list` on every rank, as in the
reference; the best model is the one with the highest `config.save_model_metric` (`lcs_precision`) of the FIRST set's result dict, and
every `config.save_interval` epochs the weights are also kept as `epoch_{n}.pth`.
Checkpoints: checkpoints/latest.pth = {epoch, time, best_metric, test_loss, lr, model_state_dict
(`module.`-prefixed), [ema_model_state_dict], optimizer_state_dict, scheduler_state_dict};
best weights (unprefixed) -> best.pth -> `{network}-metric{best:.3f}.pth` at the end.
"""
import argparse
import functools

from . import entry
from .text_scripts import test_text_recognition_for_all_dataset, train_text_recognition


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Text Recognition Training (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get training config and saving log/models')
    return parser.parse_args()


TASK = entry.TrainTask(train=train_text_recognition, best=entry.BEST_METRIC, criterion_dict=True,
                       eval_loaders=functools.partial(entry.dataset_list_loaders, collater='test_collater'),
                       validate=test_text_recognition_for_all_dataset, evaluate=entry.evaluate_first_dataset, epoch_weights=True)


def main():
    entry.train(parse_args, TASK)


if __name__ == '__main__':
    main()
