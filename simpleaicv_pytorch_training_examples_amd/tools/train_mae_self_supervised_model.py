"""torchrun entry point for MAE self-supervised pre-training on MI355X -- same CLI (`--work-dir`), same `train_config.py`
contract, same log lines and checkpoint schema as the reference tools/train_mae_self_supervised_model.py (:34-278):

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.train_mae_self_supervised_model --work-dir ./

One process per GPU; process group backend "nccl" (= RCCL over xGMI on ROCm).  No test pass: the epoch's mean training
loss selects the best weights.  Checkpoints: checkpoints/latest.pth = {epoch, time, best_loss, train_loss, lr,
model_state_dict (`module.`-prefixed), [ema_model_state_dict], optimizer_state_dict, scheduler_state_dict}; best weights
(unprefixed) -> best.pth and the encoder alone -> best_encoder.pth, renamed `{network}-loss{best:.3f}[_encoder].pth` at the
end (the encoder file is what the fine-tuning configs load through load_state_dict)."""
import argparse

from . import entry
from .scripts import train_mae_self_supervised_learning


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch MAE Self Supervised Learning Training (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get training config and saving log/models')
    return parser.parse_args()


# (the encoder alone is what the fine-tuning configs load)
TASK = entry.TrainTask(train=train_mae_self_supervised_learning, best=entry.BEST_LOSS,
                       best_files={'best.pth': lambda network: network.state_dict(),
                                   'best_encoder.pth': lambda network: network.encoder.state_dict()})


def main():
    entry.train(parse_args, TASK)


if __name__ == '__main__':
    main()
