#!/usr/bin/env python
"""The reference's two entry points on a MARS tree, through the drop-in `reid` / `utils` packages: mars_train.py's
main (get_data, the model / criterion / two-group SGD set-up, SEQTrainer epochs, ATTEvaluator + checkpoints,
mars_train.py:68-142), then test_all.py's evaluation (get_data with only_eval=True, fresh models, the best checkpoint,
dense-mode evaluate).  Run by tests/test_gpu_datasets.py as a child process:

    PYTHONPATH=.:dropin python tests/dropin_mars_flow.py -d mars --data-dir /path/with/MARS --epochs 1
"""
import argparse
import os.path as osp
import sys

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
for p in (ROOT, osp.join(ROOT, 'dropin')):
    if p not in sys.path:
        sys.path.insert(0, p)

from reid import models                                             # noqa: E402
from reid.data import get_data                                      # noqa: E402
from reid.evaluator import ATTEvaluator                             # noqa: E402
from reid.loss import OIMLoss, PairLoss                             # noqa: E402
from reid.train import SEQTrainer                                   # noqa: E402
from utils.serialization import load_checkpoint, save_cnn_checkpoint, save_siamese_checkpoint  # noqa: E402


def train(args, device):
    dataset, num_classes, train_loader, query_loader, gallery_loader = get_data(
        args.dataset, 0, args.data_dir, args.batch_size, args.seq_len, 4, args.workers, only_eval=False)
    cnn_model = models.create('resnet50_grl', num_features=2048, dropout=0, numclasses=num_classes)
    siamese_model = models.create('siamese', input_num=2048, output_num=512, class_num=2)
    siamese_model_uncorr = models.create('siamese_video', input_num=2048, output_num=512, class_num=2)
    cnn_model = torch.nn.DataParallel(cnn_model).to(device)
    siamese_model, siamese_model_uncorr = siamese_model.to(device), siamese_model_uncorr.to(device)
    criterion_corr = OIMLoss(2048, num_classes, scalar=30, momentum=0.5).to(device)
    criterion_uncorr = OIMLoss(2048, num_classes, scalar=30, momentum=0.5).to(device)
    criterion_veri = PairLoss().to(device)
    base_param_ids = set(map(id, cnn_model.module.backbone.parameters()))
    new_params = [p for p in cnn_model.parameters() if id(p) not in base_param_ids]
    param_groups = [{'params': cnn_model.module.backbone.parameters(), 'lr_mult': 1},
                    {'params': new_params, 'lr_mult': 2},
                    {'params': siamese_model.parameters(), 'lr_mult': 2},
                    {'params': siamese_model_uncorr.parameters(), 'lr_mult': 2}]
    optimizer = torch.optim.SGD(param_groups, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    evaluator = ATTEvaluator(cnn_model, siamese_model, only_eval=False)
    trainer = SEQTrainer(cnn_model, siamese_model, siamese_model_uncorr, criterion_veri, criterion_corr,
                         criterion_uncorr, osp.join(args.logs_dir, 'train_log'))
    best_top1 = 0
    for epoch in range(args.epochs):
        for g in optimizer.param_groups:
            g['lr'] = 1e-3 * (0.1 ** (epoch // 15)) * g.get('lr_mult', 1)
        trainer.train(epoch, train_loader, optimizer)
        if (epoch + 1) % 5 == 0 or (epoch + 1) == args.epochs:
            top1 = evaluator.evaluate(dataset.query, dataset.gallery, query_loader, gallery_loader, args.logs_dir,
                                      0, 0)
            is_best = top1 > best_top1 or epoch == 0
            best_top1 = max(best_top1, top1)
            save_cnn_checkpoint({'state_dict': cnn_model.state_dict(), 'epoch': epoch + 1, 'best_top1': best_top1},
                                is_best, fpath=osp.join(args.logs_dir, 'cnn_checkpoint.pth.tar'))
            save_siamese_checkpoint({'state_dict': siamese_model.state_dict(), 'epoch': epoch + 1,
                                     'best_top1': best_top1}, is_best,
                                    fpath=osp.join(args.logs_dir, 'siamese_checkpoint.pth.tar'))
    return num_classes


def test_all(args, device):
    dataset, num_classes, _, query_loader, gallery_loader = get_data(
        args.dataset, 0, args.data_dir, args.batch_size, args.seq_len, 4, args.workers, only_eval=True)
    cnn_model = models.create('resnet50_grl', num_features=2048, dropout=0, numclasses=num_classes)
    siamese_model = models.create('siamese', input_num=2048, output_num=512, class_num=2)
    cnn_model = torch.nn.DataParallel(cnn_model).to(device)
    siamese_model = siamese_model.to(device)
    evaluator = ATTEvaluator(cnn_model, siamese_model, only_eval=True)
    cnn_model.load_state_dict(load_checkpoint(osp.join(args.logs_dir, 'cnnmodel_best.pth.tar'))['state_dict'])
    siamese_model.load_state_dict(load_checkpoint(osp.join(args.logs_dir, 'siamesemodel_best.pth.tar'))['state_dict'])
    return evaluator.evaluate(dataset.query, dataset.gallery, query_loader, gallery_loader, args.logs_dir, 0, 0)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('-d', '--dataset', default='mars', choices=['mars', 'duke'])
    ap.add_argument('--data-dir', required=True)
    ap.add_argument('-b', '--batch-size', type=int, default=8)
    ap.add_argument('-j', '--workers', type=int, default=2)
    ap.add_argument('--seq_len', type=int, default=4)
    ap.add_argument('--epochs', type=int, default=1)
    ap.add_argument('--logs-dir', required=True)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    dev = torch.device('cuda:0')
    train(args, dev)
    top1 = test_all(args, dev)
    print('dropin flow ok: dense rank-1 %.4f' % top1)
