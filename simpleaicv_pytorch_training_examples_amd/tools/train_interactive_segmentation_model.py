"""torchrun entry point for SAM training on MI355X -- same CLI (`--work-dir`), same `train_config.py`
contract, log lines and checkpoint schema as the reference tools/train_interactive_segmentation_model.py
(:33-258), launched the same way:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.train_interactive_segmentation_model --work-dir ./

One process per GPU; backend "nccl" (= RCCL over xGMI on ROCm).  Checkpoints: checkpoints/latest.pth =
{epoch, time, best_loss, train_loss, lr, model_state_dict (`module.`-prefixed), optimizer_state_dict,
scheduler_state_dict}; epoch_N.pth every save_interval; best weights -> `{network}-loss{best:.3f}.pth`.
"""
import argparse

# (a captured step needs ROCm's graph packet capture OFF, and the HIP runtime reads that switch before its first call: running this
# module with `-m` imports the package -- whose __init__ sets it -- before torch is imported below)
from . import entry
from .interactive_segmentation_scripts import train_sam_segmentation


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Interactive Segmentation Training (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get training config and saving log/models')
    return parser.parse_args()


TASK = entry.TrainTask(train=train_sam_segmentation, best=entry.BEST_LOSS, ema=False, epoch_weights=True)


def main():
    entry.train(parse_args, TASK)


if __name__ == '__main__':
    main()
