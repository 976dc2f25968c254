"""torchrun entry point for text-recognition evaluation on MI355X -- same CLI (`--work-dir`), same `test_config.py` contract
and log lines as the reference tools/test_text_recognition_model.py:

    torchrun --nproc_per_node=N --master_addr 127.0.0.1 --master_port P \\
        -m simpleaicv_pytorch_training_examples_amd.tools.test_text_recognition_model --work-dir ./

    model: <network>, params: ...
    then per validation set `eval dataset:<names joined with [+]>` and one `key: value` line per entry of its result dict
    (the two per-image times, test_loss, str_acc, not_included_str_percent, final_edit_distance, lcs_precision, lcs_recall)

The reference's flops / macs line needs one input size; the images here are 32 x W with W per batch, so only the parameter count is
logged.  As in the reference the loaders are NOT sharded (every rank evaluates every set; rank 0 logs)."""
import argparse
import os
import sys

import torch
from torch.utils.data import DataLoader

from .. import engine
from .text_scripts import test_text_recognition_for_all_dataset
from .utils import get_logger, set_seed


def parse_args():
    parser = argparse.ArgumentParser(description='PyTorch Text Recognition Testing (MI355X engine)')
    parser.add_argument('--work-dir', type=str, help='path for get testing config')
    return parser.parse_args()


def main():
    assert torch.cuda.is_available(), 'need gpu to train network!'
    args = parse_args()
    sys.path.append(args.work_dir)
    from test_config import config
    log_dir = os.path.join(args.work_dir, 'log')
    config.gpus_type = torch.cuda.get_device_name()
    config.gpus_num = int(os.environ.get('WORLD_SIZE', torch.cuda.device_count()))
    set_seed(config.seed)
    local_rank = int(os.environ['LOCAL_RANK'])
    config.local_rank = local_rank
    torch.cuda.set_device(local_rank)
    torch.distributed.init_process_group(backend='nccl', init_method='env://', device_id=torch.device('cuda', local_rank))
    config.group = torch.distributed.new_group(list(range(config.gpus_num)))
    os.makedirs(log_dir, exist_ok=True)
    torch.distributed.barrier(device_ids=[local_rank])
    logger = get_logger('test', log_dir)
    info = (lambda m: logger.info(m)) if local_rank == 0 else (lambda m: None)

    assert config.batch_size % config.gpus_num == 0, 'config.batch_size is not divisible by config.gpus_num!'
    assert config.num_workers % config.gpus_num == 0, 'config.num_workers is not divisible by config.gpus_num!'
    batch_size = int(config.batch_size // config.gpus_num)
    num_workers = int(config.num_workers // config.gpus_num)
    val_loader_list = [DataLoader(dataset, batch_size=batch_size, shuffle=False, pin_memory=True, num_workers=num_workers,
                                  collate_fn=config.test_collater) for dataset in config.val_dataset_list]
    for key, value in config.__dict__.items():
        if not key.startswith('__') and key not in ['model']:
            info(f'{key}: {value}')

    model, test_criterion = config.model, config.test_criterion
    info(f'model: {config.network}, params: {sum(p.numel() for p in model.parameters())}')
    model = model.cuda()
    test_criterion = test_criterion.cuda()
    model = engine.DistributedDataParallel(model, device_ids=[local_rank], output_device=local_rank, process_group=config.group)
    result_dict = test_text_recognition_for_all_dataset(val_loader_list, model, test_criterion, config)
    for name, per_dataset in result_dict.items():
        log_info = f'eval dataset:{name}\n'
        for key, value in per_dataset.items():
            log_info += f'{key}: {value}\n'
        info(log_info)
    torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
