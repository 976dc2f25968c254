"""torchrun entry point for detection (DETR) training on MI355X -- same CLI (`--work-dir`), same
`train_config.py` contract and training log lines as the reference tools/train_detection_model.py,
launched the same way:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.train_detection_model --work-dir ./

One process per GPU; backend "nccl" (= RCCL over xGMI on ROCm).  The evaluation pass the reference runs at
`config.eval_epoch` is not wired into this entry script -- its COCO form needs pycocotools, which the image does not
have; `tools.scripts.test_detection` provides the VOC form (decoders + mAP, pinned to the reference's result dict in
tests/test_host_logic.py) for callers that want it -- so the best model is tracked on the training loss.  Checkpoints: checkpoints/latest.pth = {epoch, time,
best_loss, train_loss, lr, model_state_dict (`module.`-prefixed), optimizer_state_dict, scheduler_state_dict}.
"""
import argparse

from . import entry
from .scripts import train_detection


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Detection Training (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get training config and saving log/models')
    return parser.parse_args()


# config.ema_model is kept for the loop, but the checkpoints hold model.module and no EMA key
TASK = entry.TrainTask(train=train_detection, best=entry.BEST_LOSS, ema=False)


def main():
    entry.train(parse_args, TASK)


if __name__ == '__main__':
    main()
