#!/usr/bin/env python
"""Cluster-contrast training without labels on a synthetic re-id task: the flow of examples/train_synthetic.py (same
factory calls, two-group SGD, trainer and evaluator) with the pids hidden from training.  Every epoch the evaluator
extracts the training tracklets' features, `pseudo_labels` clusters them, the two `ClusterMemoryLoss` memories are seeded
from the cluster centroids and SEQTrainer trains on the relabelled tracklets (grl_amd.reid.train.pseudo.train_unsupervised).
The hidden pids are only used to print how good the clusters were.  Run:

    PYTHONPATH=.:dropin python examples/train_unsupervised_synthetic.py --epochs 2
    PYTHONPATH=.:dropin python examples/train_unsupervised_synthetic.py --epochs 2 --camera-proxies --k-neg 8 --inter-from-epoch 1

    PYTHONPATH=.:dropin python examples/train_unsupervised_synthetic.py --epochs 2 --hybrid-memory --self-paced 0.02
    PYTHONPATH=.:dropin python examples/train_unsupervised_synthetic.py --epochs 2 --mean-teacher 0.999 --soft-weight 0.5 --eval-teacher
    PYTHONPATH=.:dropin python examples/train_unsupervised_synthetic.py --epochs 2 --mean-teacher 0.999 --soft-weight 0.5 --soft-tri-weight 0.8
    PYTHONPATH=.:dropin python examples/train_unsupervised_synthetic.py --epochs 2 --mean-teacher 0.999 --soft-weight 0.5 --ins-hard-weight 1 --ins-soft-weight 0.4

(the second form: camera-aware proxies, one memory row per cluster and camera -- ProxyMemoryLoss under CameraSEQTrainer;
the third: a hybrid memory with one row per tracklet, the samples the clustering calls noise trained on as classes of their
own, and only the clusters that are stable under eps -/+ 0.02 kept -- HybridMemoryLoss under HybridSEQTrainer, DESIGN.md 4ak;
the fourth: a mean teacher -- an averaged copy of the model whose softmax over the cluster memory is a soft target next to
the hard cluster id, SoftClusterMemoryLoss under MeanTeacherSEQTrainer, and with --eval-teacher the model that is evaluated
and clustered with; the fifth: the teacher's distances at the student's batch-hard indices as a soft target of
the triplet term too, SoftTripletLoss; the sixth: the hard instance contrast and the soft instance consistency
of the batch's rows against the teacher's, InstanceContrastLoss)

Every identity is a low-frequency colour layout ("a person in front of a background", as grl_amd.synthetic.
synth_clips_structured); a tracklet is a small deviation from its identity's layout, a frame a smaller one, plus pixel noise.
Single process: under torch.distributed the flow is the same on every rank (the evaluator gathers the features)."""
import argparse
import os.path as osp
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, Dataset

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
for p in (ROOT, osp.join(ROOT, 'dropin')):
    if p not in sys.path:
        sys.path.insert(0, p)

from reid import models                                             # noqa: E402
from reid.loss import PairLoss, ClusterMemoryLoss, ProxyMemoryLoss, HybridMemoryLoss, SoftClusterMemoryLoss  # noqa: E402
from reid.train import (SEQTrainer, CameraSEQTrainer, HybridSEQTrainer, MeanTeacher, MeanTeacherSEQTrainer,   # noqa: E402
                        train_unsupervised)
from reid.evaluator import ATTEvaluator                             # noqa: E402
from reid.data import RandomPairSamplerForMars                      # noqa: E402
from grl_amd.synthetic import synth_state_dict, IMAGENET_MEAN, IMAGENET_STD   # noqa: E402


def identity_clip(pid, track, seq_len, seed, h=256, w=128):
    """float32 [T,3,h,w], ToTensor + Normalize applied: identity layout + tracklet deviation + frame deviation + noise"""
    base = np.random.Generator(np.random.PCG64([seed, pid])).uniform(0.0, 1.0, (1, 3, 8, 4))
    g = np.random.Generator(np.random.PCG64([seed, pid, track + 1]))
    low = base + g.uniform(-0.08, 0.08, (1, 3, 8, 4)) + g.uniform(-0.05, 0.05, (seq_len, 3, 8, 4))
    low = F.interpolate(torch.from_numpy(low.astype(np.float32)), size=(h, w), mode='bilinear', align_corners=False)
    noise = torch.from_numpy(g.uniform(-0.1, 0.1, (seq_len, 3, h, w)).astype(np.float32))
    x = ((low + noise).clamp_(0.0, 1.0) * 255.0).round_().div_(255.0)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).view(1, 3, 1, 1)
    return x.sub_(mean).div_(std)


def tracklets_of(pids, per_cam, cams, first_track=0):
    """[((pid, track), pid, cam)]: the first element stands for a tracklet's frame paths"""
    return [((pid, first_track + c * per_cam + t), pid, c) for pid in pids for c in cams for t in range(per_cam)]


class Clips(Dataset):
    """``index=True``: every item ends with its dataset index, as RawVideoDataset(index=True) -- the sample's memory row"""

    def __init__(self, tracklets, seq_len, seed, index=False):
        self.tracklets, self.seq_len, self.seed, self.index = list(tracklets), seq_len, seed, index

    def __len__(self):
        return len(self.tracklets)

    def __getitem__(self, i):
        (pid, track), label, cam = self.tracklets[i]
        item = (identity_clip(pid, track, self.seq_len, self.seed), label, cam)
        return item + (torch.tensor(i, dtype=torch.int64),) if self.index else item


def refuse_conflicts(args):
    """SystemExit with a message for flags that exclude each other, before anything is built"""
    if args.camera_proxies and args.hybrid_memory:
        raise SystemExit('--camera-proxies and --hybrid-memory exclude each other')
    if args.self_paced is not None and not args.hybrid_memory:
        raise SystemExit('--self-paced needs --hybrid-memory')
    if args.mean_teacher is None and (args.eval_teacher or args.soft_weight is not None):
        raise SystemExit('--soft-weight and --eval-teacher need --mean-teacher ALPHA')
    if args.mean_teacher is None and getattr(args, 'soft_tri_weight', None) is not None:
        raise SystemExit('--soft-tri-weight needs --mean-teacher ALPHA')
    for flag in ('ins_hard_weight', 'ins_soft_weight', 'ins_tau'):
        if args.mean_teacher is None and getattr(args, flag, None) is not None:
            raise SystemExit('--%s needs --mean-teacher ALPHA' % flag.replace('_', '-'))
    if args.mean_teacher is not None and (args.camera_proxies or args.hybrid_memory):
        raise SystemExit('--mean-teacher is built for the plain cluster memory: it excludes --camera-proxies and '
                         '--hybrid-memory (DESIGN.md 4al, out of scope)')


def main(args):
    refuse_conflicts(args)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    device = torch.device('cuda', 0)
    train = tracklets_of(range(args.ids), args.per_cam, (0, 1))
    hidden = np.array([t[1] for t in train])
    train = [(paths, -1, cam) for paths, _, cam in train]                        # the pids are hidden from here on
    test_ids = range(1000, 1000 + args.test_ids)
    query, gallery = tracklets_of(test_ids, 1, (0,)), tracklets_of(test_ids, 2, (1, 2), first_track=10)
    query_loader = DataLoader(Clips(query, args.seq_len, args.seed), batch_size=8)
    gallery_loader = DataLoader(Clips(gallery, args.seq_len, args.seed), batch_size=8)

    cnn_model = models.create('resnet50_grl', num_features=2048, dropout=0, numclasses=args.ids, pretrained=False)
    siamese_model = models.create('siamese', input_num=2048, output_num=512, class_num=2)
    siamese_model_uncorr = models.create('siamese_video', input_num=2048, output_num=512, class_num=2)
    cnn_model.load_state_dict(synth_state_dict(cnn_model, seed=0))
    siamese_model.load_state_dict(synth_state_dict(siamese_model, seed=0, prefix='siamese.'))
    siamese_model_uncorr.load_state_dict(synth_state_dict(siamese_model_uncorr, seed=0, prefix='siamese_video.'))
    cnn_model, siamese_model, siamese_model_uncorr = (m.to(device) for m in (cnn_model, siamese_model, siamese_model_uncorr))

    # the memories are seeded every epoch (reset): the size given here is only a placeholder
    if args.hybrid_memory:
        # one memory row per tracklet, DESIGN.md 4ak: the trainer that keeps the batch's instance indices
        criterion_corr, criterion_uncorr = (HybridMemoryLoss(2048, temp=args.temp, momentum=args.momentum).to(device)
                                            for _ in range(2))
    elif args.camera_proxies:
        # one memory row per (cluster, camera) pair, DESIGN.md 4aj: the trainer that keeps the batch's camera ids
        criterion_corr, criterion_uncorr = (ProxyMemoryLoss(2048, temp=args.temp, momentum=args.momentum, mode=args.mode,
                                                            k_neg=args.k_neg).to(device) for _ in range(2))
    else:
        # (with a mean teacher: the criterion that takes the teacher's rows as a soft target)
        crit = SoftClusterMemoryLoss if args.mean_teacher is not None else ClusterMemoryLoss
        criterion_corr = crit(2048, 2, temp=args.temp, momentum=args.momentum, mode=args.mode).to(device)
        criterion_uncorr = crit(2048, 2, temp=args.temp, momentum=args.momentum, mode=args.mode).to(device)
    criterion_veri = PairLoss().to(device)

    base_param_ids = set(map(id, cnn_model.backbone.parameters()))
    new_params = [p for p in cnn_model.parameters() if id(p) not in base_param_ids]
    param_groups = [{'params': cnn_model.backbone.parameters(), 'lr_mult': 1}, {'params': new_params, 'lr_mult': 2},
                    {'params': siamese_model.parameters(), 'lr_mult': 2},
                    {'params': siamese_model_uncorr.parameters(), 'lr_mult': 2}]
    optimizer = torch.optim.SGD(param_groups, lr=args.lr, momentum=0.9, weight_decay=5e-4, nesterov=True)
    for g in optimizer.param_groups:
        g['lr'] = args.lr * g.get('lr_mult', 1)

    evaluator = ATTEvaluator(cnn_model, siamese_model, only_eval=False)
    if args.mean_teacher is not None:
        teacher = MeanTeacher(cnn_model, siamese_model, alpha=args.mean_teacher)
        trainer = MeanTeacherSEQTrainer(cnn_model, siamese_model, siamese_model_uncorr, criterion_veri, criterion_corr,
                                        criterion_uncorr, osp.join(args.logs_dir, 'train_log'), teacher=teacher,
                                        soft_weight=0.5 if args.soft_weight is None else args.soft_weight,
                                        tri_soft_weight=0.0 if args.soft_tri_weight is None else args.soft_tri_weight,
                                        ins_hard_weight=0.0 if args.ins_hard_weight is None else args.ins_hard_weight,
                                        ins_soft_weight=0.0 if args.ins_soft_weight is None else args.ins_soft_weight,
                                        ins_tau=0.1 if args.ins_tau is None else args.ins_tau)
        teacher_evaluator = ATTEvaluator(*teacher.models, only_eval=False)
        if args.eval_teacher:                                # the teacher's features are clustered, and it is what is scored
            evaluator, student_evaluator = teacher_evaluator, evaluator
    else:
        trainer = (HybridSEQTrainer if args.hybrid_memory else CameraSEQTrainer if args.camera_proxies else SEQTrainer)(
            cnn_model, siamese_model, siamese_model_uncorr, criterion_veri, criterion_corr, criterion_uncorr,
            osp.join(args.logs_dir, 'train_log'))

    def make_eval_loader(tracklets):
        return DataLoader(Clips(tracklets, args.seq_len, args.seed), batch_size=8, shuffle=False)

    def make_train_loader(relabelled):
        return DataLoader(Clips(relabelled, args.seq_len, args.seed, index=args.hybrid_memory), batch_size=args.batch_size,
                          sampler=RandomPairSamplerForMars(relabelled), drop_last=True)

    def on_epoch(epoch, labels):
        s = labels.pair_scores(hidden)
        if args.hybrid_memory:
            print('epoch {}: {} instances in {} classes'.format(epoch, criterion_corr.num_instances, criterion_corr.num_classes))
        if args.camera_proxies:
            print('epoch {}: {} proxies, inter-camera term {}'.format(epoch, criterion_corr.num_proxies,
                                                                      'on' if criterion_corr.inter_on else 'off'))
        print('epoch {}: n_clusters {} n_noise {} of {} | against the hidden pids: precision {:.3f} recall {:.3f} F1 {:.3f} '
              'ARI {:.3f} | loss {:.3f}'.format(epoch, labels.n_clusters, labels.n_noise, len(labels), s['precision'],
                                                s['recall'], s['f1'], s['ari'], trainer.meters['loss'].avg))
        if args.mean_teacher is not None:
            print('epoch {}: teacher after {} updates, alpha {}'.format(epoch, teacher.step, teacher.alpha))
            other = student_evaluator if args.eval_teacher else teacher_evaluator
            print('the {}:'.format('student' if args.eval_teacher else 'teacher'))
            other.evaluate(None, None, query_loader, gallery_loader, args.logs_dir, False, False)
            print('the {}:'.format('teacher' if args.eval_teacher else 'student'))
        evaluator.evaluate(None, None, query_loader, gallery_loader, args.logs_dir, False, False)   # prints Mean AP / Rank-k

    print('before training:')
    evaluator.evaluate(None, None, query_loader, gallery_loader, args.logs_dir, False, False)
    label_kwargs = dict(method=args.method, eps=args.eps, min_samples=args.min_samples, k1=args.k1, k2=args.k2, k=args.k,
                        min_cluster_size=args.min_cluster_size)
    train_unsupervised(trainer, evaluator, optimizer, train, make_eval_loader, make_train_loader, args.epochs,
                       label_kwargs=label_kwargs, on_epoch=on_epoch, cameras=args.camera_proxies,
                       inter_from_epoch=args.inter_from_epoch, hybrid=args.hybrid_memory,
                       self_paced=None if args.self_paced is None else dict(
                           delta=args.self_paced, method=args.method, eps=args.eps, min_samples=args.min_samples, k1=args.k1,
                           k2=args.k2))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--ids', type=int, default=12, help='training identities (hidden)')
    ap.add_argument('--per-cam', type=int, default=3, help='tracklets per identity and camera (two cameras)')
    ap.add_argument('--test-ids', type=int, default=8)
    ap.add_argument('-b', '--batch-size', type=int, default=8)
    ap.add_argument('--seq_len', type=int, default=4)
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--method', default='jaccard', choices=['jaccard', 'cosine', 'hdbscan', 'kmeans'])
    ap.add_argument('--eps', type=float, default=0.5)
    ap.add_argument('--min-samples', type=int, default=2)
    ap.add_argument('--k1', type=int, default=5)
    ap.add_argument('--k2', type=int, default=1)
    ap.add_argument('--k', type=int, default=None, help="clusters of method 'kmeans'")
    ap.add_argument('--min-cluster-size', type=int, default=3)
    ap.add_argument('--temp', type=float, default=0.05)
    ap.add_argument('--momentum', type=float, default=0.2)
    ap.add_argument('--mode', default='hard', choices=['hard', 'mean', 'instance'])
    ap.add_argument('--camera-proxies', action='store_true',
                    help='camera-aware proxies: ProxyMemoryLoss under CameraSEQTrainer (DESIGN.md 4aj)')
    ap.add_argument('--k-neg', type=int, default=50, help='hardest proxies of other clusters in the inter-camera term')
    ap.add_argument('--inter-from-epoch', type=int, default=0, help='first epoch with the inter-camera term')
    ap.add_argument('--hybrid-memory', action='store_true',
                    help='hybrid memory: HybridMemoryLoss under HybridSEQTrainer, noise samples stay in the epoch (DESIGN.md 4ak)')
    ap.add_argument('--self-paced', type=float, default=None, metavar='DELTA',
                    help="with --hybrid-memory and --method jaccard / cosine: keep only the clusters stable under eps -/+ DELTA")
    ap.add_argument('--mean-teacher', type=float, default=None, metavar='ALPHA',
                    help='mean teacher with this EMA coefficient: SoftClusterMemoryLoss under MeanTeacherSEQTrainer (DESIGN.md 4al)')
    ap.add_argument('--soft-weight', type=float, default=None, metavar='W',
                    help="with --mean-teacher: weight of the teacher's softmax in the identity losses (default 0.5)")
    ap.add_argument('--soft-tri-weight', type=float, default=None, metavar='W',
                    help="with --mean-teacher: weight of the teacher's soft target in the batch-hard triplet term, SoftTripletLoss "
                         '(DESIGN.md 4am; default 0: the hard triplet)')
    ap.add_argument('--ins-hard-weight', type=float, default=None, metavar='W',
                    help="with --mean-teacher: weight of the hard instance contrast against the teacher's rows, "
                         'InstanceContrastLoss (DESIGN.md 4ao; default 0: off)')
    ap.add_argument('--ins-soft-weight', type=float, default=None, metavar='W',
                    help='with --mean-teacher: weight of the soft instance consistency (default 0: off)')
    ap.add_argument('--ins-tau', type=float, default=None, metavar='T',
                    help='with --mean-teacher: temperature of both instance terms (default 0.1)')
    ap.add_argument('--eval-teacher', action='store_true',
                    help='with --mean-teacher: evaluate and cluster with the teacher (ATTEvaluator on teacher.models)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--logs-dir', type=str, default='/tmp/grl_logs')
    main(ap.parse_args())
