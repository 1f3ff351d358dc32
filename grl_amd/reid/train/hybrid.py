"""SEQTrainer that carries every row's instance index -- its row of the hybrid memory -- to its identity criteria (DESIGN.md
4ak): what ``HybridMemoryLoss`` needs and ``SEQTrainer`` has no place for.  The step is SEQTrainer's own -- the same forward,
losses and launches; ``_parse_data`` takes the batch's LAST element (``RawVideoDataset(index=True)``) off before the base
sees the batch, and ``_id_extra`` adds ``index=`` in the row order of the targets it is given."""
import torch

from grl_amd import dist as grl_dist
from grl_amd.reid.train.trainer import SEQTrainer


class HybridSEQTrainer(SEQTrainer):
    """``criterion_corr`` / ``criterion_uncorr`` are called as ``criterion(feats, targets, index=index)``."""

    def _parse_data(self, inputs):
        """as SEQTrainer on the batch without its last element, and the batch's instance indices in the two row orders of
        ``_forward``'s targets: 'clip' = probe-then-gallery, 'frame' = expanded over T; gathered in rank order under
        GRL_DP_GLOBAL_HEADS.  Built here, on the launch stream and before ``_forward`` forks its side stream, which reads them."""
        index = inputs[-1] if len(inputs) > 3 else None
        if not (torch.is_tensor(index) and index.dtype == torch.int64 and index.dim() == 1
                and index.size(0) == inputs[0].size(0)):
            raise ValueError('HybridSEQTrainer: the last element of a batch must be the int64 [%d] instance indices of its '
                             'clips (got %s): build the loader on RawVideoDataset(index=True)' % (
                                 inputs[0].size(0), '%s %s' % (index.dtype, tuple(index.shape)) if torch.is_tensor(index)
                                 else 'a batch of %d elements' % len(inputs) if index is None else type(index).__name__))
        index = index.to(self.device)
        if grl_dist.global_heads():
            index = grl_dist.gather_global(index)
        b, seq_len = index.size(0), inputs[0].size(1)
        pairs = index.view(b // 2, -1)
        self._index_rows = {'clip': torch.cat((pairs[:, 0], pairs[:, 1])),
                            'frame': index.unsqueeze(1).expand(b, seq_len).reshape(-1)}
        return super(HybridSEQTrainer, self)._parse_data(tuple(inputs[:-1]))

    def _id_extra(self, rows):
        return {'index': self._index_rows[rows]}
