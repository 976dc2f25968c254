"""The one driver behind every `tools/train_*_model.py` and `tools/test_*_model*.py` entry module.

An entry module keeps its docstring (the task's checkpoint schema and launch line), its `parse_args()` and a `TASK`: a `TrainTask` /
`TestTask` that carries only what differs between tasks.  `main()` hands both to `train()` / `test()` below, which run the steps of the
reference's entry scripts in the reference's order: process setup, loaders, preamble logging, resume, the epoch loop (`fit`), or the one
evaluation and its report.  `resume()` and `fit()` call nothing of torch.cuda or torch.distributed: tests/test_entry_host.py drives them
on the CPU with stand-ins, task by task.  A new task is a `TASK` and a thin module, not a copy of one of these functions.
"""
import collections
import dataclasses
import functools
import importlib
import os
import sys
import time
import typing

import torch
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from .. import engine
from .salient_object_detection_scripts import first_dataset_metric
from .utils import (Scheduler, build_optimizer, build_training_mode, compute_macs_and_params, get_logger, set_seed,
                    worker_seed_init_fn)

# ------------------------------------------------------------------------------------------------ what "best" means, and its spelling
# key: its name in latest.pth and in the log lines; tag: the best file is `{network}-{tag}{best:.3f}.pth`; start: the value before the
# first epoch; better(score, best); second: the other number latest.pth keeps (read back on resume); show: how the log lines print the
# best value; resume_second: how the resume line prints `second` (each family has its own spelling, the reference's).
Best = collections.namedtuple('Best', 'key tag start better second show resume_second')


def _higher(score, best):
    return score > best and score <= 100


def _lower(score, best):
    return score < best


BEST_ACC1 = Best('best_acc1', 'acc', 0, _higher, 'test_loss', '{:.3f}%', ', test_loss: {:.4f}')
BEST_METRIC_PERCENT = Best('best_metric', 'metric', 0, _higher, 'test_loss', '{:.3f}%', ', test_loss: {:.4f}')
BEST_METRIC = Best('best_metric', 'metric', 0, _higher, 'test_loss', '{:.3f}', ', test_loss: {}')
BEST_LOSS = Best('best_loss', 'loss', 1e9, _lower, 'train_loss', '{:.4f}', '')      # no evaluation: the epoch's training loss decides


# ------------------------------------------------------------------------------------------------ the task descriptions
@dataclasses.dataclass(frozen=True)
class TrainTask:
    train: typing.Callable                      # the loop: (train_loader, model, criterion, optimizer, scheduler, epoch, logger, config)
    best: Best
    criterion_dict: bool = False                # config.train_criterion is {name: module}, not a module
    # With an evaluation (all three or none; config.test_criterion exists exactly then): eval_loaders(config, make) builds the
    # loader(s), validate(loaders, model, test_criterion, config) is the loop library's function, and
    # evaluate(run, config, epoch, info, score, test_loss) -> (score, test_loss) decides when to call run(), what to log and what to keep.
    eval_loaders: typing.Optional[typing.Callable] = None
    validate: typing.Optional[typing.Callable] = None
    evaluate: typing.Optional[typing.Callable] = None
    ema: bool = True                            # best / epoch weights come from the EMA model under config.use_ema_model, and latest.pth
    #                                             keeps `ema_model_state_dict`; False: always model.module, no EMA key
    epoch_weights: bool = False                 # also keep epoch_{n}.pth every config.save_interval epochs
    # file name -> state dict of the best network; every one is renamed `{network}-{tag}{best:.3f}` + what follows `best` at the end
    best_files: typing.Mapping = dataclasses.field(default_factory=lambda: {'best.pth': lambda network: network.state_dict()})


@dataclasses.dataclass(frozen=True)
class TestTask:
    validate: typing.Callable                   # (loaders, model, *extra_args(config), config) -> result
    eval_loaders: typing.Callable               # (config, make) -> loader(s)
    report: typing.Callable                     # (result, config, info): the log block of the result
    extra_args: typing.Callable = lambda config: (config.test_criterion.cuda(), )
    describe: typing.Callable = lambda config, model: 'flops: {}, macs: {}, params: {}'.format(*compute_macs_and_params(config, model))


# ------------------------------------------------------------------------------------------------ process setup
def setup(parse_args, kind):
    """-> (config, logger, info, local_rank, work_dir) for kind 'train' | 'test', with the process group up and `log/` made."""
    assert torch.cuda.is_available(), 'need gpu to train network!'
    work_dir = parse_args().work_dir
    sys.path.append(work_dir)
    config = importlib.import_module(f'{kind}_config').config
    log_dir = os.path.join(work_dir, 'log')
    config.gpus_type = torch.cuda.get_device_name()
    config.gpus_num = int(os.environ.get('WORLD_SIZE', torch.cuda.device_count()))
    # set_seed() allocates the deterministic workspaces on the current device, which is still device 0 on every rank
    # here; it belongs after set_device(local_rank).  Kept in the reference's order until that fix lands with its own world-2 test.
    set_seed(config.seed)
    local_rank = int(os.environ['LOCAL_RANK'])
    config.local_rank = local_rank
    torch.cuda.set_device(local_rank)
    torch.distributed.init_process_group(backend='nccl', init_method='env://', device_id=torch.device('cuda', local_rank))
    config.group = torch.distributed.new_group(list(range(config.gpus_num)))
    if kind == 'train':
        os.makedirs(os.path.join(work_dir, 'checkpoints'), exist_ok=True)
    os.makedirs(log_dir, exist_ok=True)
    torch.distributed.barrier(device_ids=[local_rank])
    logger = get_logger(kind, log_dir)
    return config, logger, rank0_info(logger, local_rank), local_rank, work_dir


def rank0_info(logger, local_rank):
    return (lambda m: logger.info(m)) if local_rank == 0 else (lambda m: None)


# ------------------------------------------------------------------------------------------------ loaders
def per_rank_sizes(config):
    assert config.batch_size % config.gpus_num == 0, 'config.batch_size is not divisible by config.gpus_num!'
    assert config.num_workers % config.gpus_num == 0, 'config.num_workers is not divisible by config.gpus_num!'
    return int(config.batch_size // config.gpus_num), int(config.num_workers // config.gpus_num)


def train_loader_of(config, batch_size, num_workers, local_rank):
    init_fn = functools.partial(worker_seed_init_fn, num_workers=num_workers, local_rank=local_rank, seed=config.seed)
    train_sampler = DistributedSampler(config.train_dataset, shuffle=True)
    return DataLoader(config.train_dataset, batch_size=batch_size, shuffle=False, pin_memory=True, drop_last=True,
                      num_workers=num_workers, collate_fn=config.train_collater, sampler=train_sampler, worker_init_fn=init_fn)


def eval_loader(dataset, collater, batch_size, num_workers, sampler=None):
    return DataLoader(dataset, batch_size=batch_size, shuffle=False, pin_memory=True, num_workers=num_workers, collate_fn=collater,
                      sampler=sampler)


def sharded_test_loader(config, make):          # classification: every rank evaluates its shard
    return make(config.test_dataset, config.test_collater, sampler=DistributedSampler(config.test_dataset, shuffle=False))


def whole_test_loader(config, make):            # every rank evaluates the whole set
    return make(config.test_dataset, config.test_collater)


def dataset_list_loaders(config, make, collater='val_collater'):
    return [make(dataset, getattr(config, collater)) for dataset in config.val_dataset_list]


# ------------------------------------------------------------------------------------------------ preamble logging
def log_config(config, info):
    for key, value in config.__dict__.items():
        if not key.startswith('__') and key not in ['model']:
            info(f'{key}: {value}')


def log_parameters_and_buffers(model, info):
    info('--------------------parameters--------------------')
    for name, param in model.named_parameters():
        info(f'name: {name}, grad: {param.requires_grad}')
    info('--------------------buffers--------------------')
    for name, buffer in model.named_buffers():
        info(f'name: {name}, grad: {buffer.requires_grad}')


def log_weight_decay(model_layer_weight_decay_list, info):
    info('-------------layers weight decay---------------')
    for per_layer_list in model_layer_weight_decay_list:
        lr_scale = per_layer_list.get('lr_scale', 'not setting!')
        for name in per_layer_list['name']:
            info(f"name: {name}, lr: {per_layer_list['lr']}, weight_decay: {per_layer_list['weight_decay']}, "
                 f'lr_scale: {lr_scale}')


def log_block(info, head, result):
    """one log record: the head line, then one `key: value` line per entry"""
    info(head + '\n' + ''.join(f'{key}: {value}\n' for key, value in result.items()))


# ------------------------------------------------------------------------------------------------ evaluation during training
def eval_due(epoch, config):
    return epoch in config.eval_epoch or epoch == config.epochs


def evaluate_first_dataset(run, config, epoch, info, metric, test_loss):
    """config.val_dataset_list: the first dataset of the config is the complete validation set: it decides the checkpoint"""
    if eval_due(epoch, config):
        total_result, metric, test_loss = first_dataset_metric(run(), config.save_model_metric, metric, test_loss)
        if total_result:
            log_block(info, f'eval: epoch: {epoch:0>3d}', total_result)
    return float(metric), test_loss                      # (a numpy float32: latest.pth holds plain numbers)


# ------------------------------------------------------------------------------------------------ resume, and the epoch state machine
def _network(task, model, config):
    return config.ema_model.ema_model.module if task.ema and config.use_ema_model else model.module


def resume(task, resume_model, model, optimizer, scheduler, config, info):
    """-> (start_epoch, train_time, best, second), from latest.pth where there is one"""
    start_epoch, train_time, best, second = 1, 0, task.best.start, 0
    if os.path.exists(resume_model):
        checkpoint = torch.load(resume_model, map_location=torch.device('cpu'), weights_only=True)
        model.load_state_dict(checkpoint['model_state_dict'])
        optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
        scheduler.load_state_dict(checkpoint['scheduler_state_dict'])
        saved_epoch = checkpoint['epoch']
        start_epoch += saved_epoch
        used_time = checkpoint['time']
        train_time += used_time
        best, second, lr = checkpoint[task.best.key], checkpoint[task.best.second], checkpoint['lr']
        info(f'resuming model from {resume_model}. resume_epoch: {saved_epoch:0>3d}, used_time: {used_time:.3f} hours, '
             f'{task.best.key}: {task.best.show.format(best)}{task.best.resume_second.format(second)}, lr: {lr:.6f}')
        if task.ema and 'ema_model_state_dict' in checkpoint.keys():
            config.ema_model.ema_model.load_state_dict(checkpoint['ema_model_state_dict'])
        from .. import ops
        ops.bump_weights_epoch()
    return start_epoch, train_time, best, second


def fit(task, model, optimizer, scheduler, train_loader, eval_loaders, train_criterion, test_criterion, logger, checkpoint_dir,
        local_rank, config, start):
    """Epochs start_epoch .. config.epochs: train, evaluate where the task does, keep best.pth / latest.pth / epoch_N.pth on rank 0,
    and give the best file(s) their final name.  `start` is what resume() returned."""
    info = rank0_info(logger, local_rank)
    start_epoch, train_time, best, second = start
    score = 0
    shown = lambda: f'{task.best.key}: {task.best.show.format(best)}'  # noqa: E731
    for epoch in range(start_epoch, config.epochs + 1):
        per_epoch_start_time = time.time()
        info(f'epoch {epoch:0>3d} lr: {scheduler.current_lr:.6f}')
        train_loader.sampler.set_epoch(epoch)
        train_loss = task.train(train_loader, model, train_criterion, optimizer, scheduler, epoch, logger, config)
        info(f'train: epoch {epoch:0>3d}, train_loss: {train_loss:.4f}')
        if task.evaluate is None:
            score = second = train_loss
        else:
            run = functools.partial(task.validate, eval_loaders, model, test_criterion, config)
            score, second = task.evaluate(run, config, epoch, info, score, second)
        train_time += (time.time() - per_epoch_start_time) / 3600
        if local_rank == 0:
            if task.epoch_weights and epoch % config.save_interval == 0:
                torch.save(_network(task, model, config).state_dict(), os.path.join(checkpoint_dir, f'epoch_{epoch}.pth'))
            if task.best.better(score, best):
                best = score
                for name, state_dict_of in task.best_files.items():
                    torch.save(state_dict_of(_network(task, model, config)), os.path.join(checkpoint_dir, name))
            ckpt = {'epoch': epoch, 'time': train_time, task.best.key: best, task.best.second: second,
                    'lr': scheduler.current_lr, 'model_state_dict': model.state_dict(),
                    'optimizer_state_dict': optimizer.state_dict(), 'scheduler_state_dict': scheduler.state_dict()}
            if task.ema and config.use_ema_model:
                ckpt['ema_model_state_dict'] = config.ema_model.ema_model.state_dict()
            torch.save(ckpt, os.path.join(checkpoint_dir, 'latest.pth'))
        info(f'until epoch: {epoch:0>3d}, {shown()}')

    if local_rank == 0:
        for name in task.best_files:
            if os.path.exists(os.path.join(checkpoint_dir, name)):
                os.rename(os.path.join(checkpoint_dir, name), os.path.join(
                    checkpoint_dir, f'{config.network}-{task.best.tag}{best:.3f}{name[len("best"):]}'))
    info(f'train done. model: {config.network}, train time: {train_time:.3f} hours, {shown()}')


# ------------------------------------------------------------------------------------------------ the two drivers
def train(parse_args, task):
    config, logger, info, local_rank, work_dir = setup(parse_args, 'train')
    checkpoint_dir = os.path.join(work_dir, 'checkpoints')
    batch_size, num_workers = per_rank_sizes(config)
    train_loader = train_loader_of(config, batch_size, num_workers, local_rank)
    make = functools.partial(eval_loader, batch_size=batch_size, num_workers=num_workers)
    eval_loaders = task.eval_loaders(config, make) if task.evaluate else None
    log_config(config, info)

    model = config.model.cuda()
    if task.criterion_dict:
        train_criterion = {name: loss.cuda() for name, loss in config.train_criterion.items()}
    else:
        train_criterion = config.train_criterion.cuda()
    test_criterion = config.test_criterion.cuda() if task.evaluate else None
    log_parameters_and_buffers(model, info)
    optimizer, model_layer_weight_decay_list = build_optimizer(config, model)
    log_weight_decay(model_layer_weight_decay_list, info)
    scheduler = Scheduler(config, optimizer)
    model, config.ema_model, config.scaler = build_training_mode(config, model)
    start = resume(task, os.path.join(checkpoint_dir, 'latest.pth'), model, optimizer, scheduler, config, info)

    info(f'using torch version:{torch.__version__}')
    # torch.compile (Inductor -> Triton) is not part of the MI355X-native path; the fused HIP
    # kernels and the launch graph replace it.  `use_compile` is accepted and ignored.
    config.compile_support = False
    config.use_compile = False
    fit(task, model, optimizer, scheduler, train_loader, eval_loaders, train_criterion, test_criterion, logger, checkpoint_dir,
        local_rank, config, start)
    torch.distributed.destroy_process_group()


def test(parse_args, task):
    config, logger, info, local_rank, _ = setup(parse_args, 'test')
    batch_size, num_workers = per_rank_sizes(config)
    loaders = task.eval_loaders(config, functools.partial(eval_loader, batch_size=batch_size, num_workers=num_workers))
    log_config(config, info)

    model = config.model
    info(f'model: {config.network}, {task.describe(config, model)}')
    model = model.cuda()
    extra_args = task.extra_args(config)
    model = engine.DistributedDataParallel(model, device_ids=[local_rank], output_device=local_rank, process_group=config.group)
    task.report(task.validate(loaders, model, *extra_args, config), config, info)
    torch.distributed.destroy_process_group()


def report_result(result_dict, config, info):
    log_block(info, 'eval result:', result_dict)


def report_datasets(result_dict, config, info):
    for name, per_dataset in result_dict.items():
        log_block(info, f'eval dataset:{name}', per_dataset)
