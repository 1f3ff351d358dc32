"""SEQTrainer that carries every row's camera id to its identity criteria: what ``ProxyMemoryLoss`` needs and
``SEQTrainer`` drops.  The step is SEQTrainer's own -- the same forward, losses and launches; only ``_parse_data`` keeps
``inputs[2]`` and ``_id_extra`` adds ``cams=`` in the row order of the targets it is given."""
import torch

from grl_amd import dist as grl_dist
from grl_amd.reid.train.trainer import SEQTrainer


class CameraSEQTrainer(SEQTrainer):
    """``criterion_corr`` / ``criterion_uncorr`` are called as ``criterion(feats, targets, cams=cams)``."""

    def _parse_data(self, inputs):
        """as SEQTrainer, and the batch's cameras in the two row orders of ``_forward``'s targets: 'clip' = probe-then-gallery
        (the ``view(B / 2, -1)`` split of ``target``), 'frame' = expanded over T; gathered in rank order under
        GRL_DP_GLOBAL_HEADS.  Built here, on the launch stream and before ``_forward`` forks its side stream, which reads them."""
        cams = inputs[2]
        if not torch.is_tensor(cams):
            cams = torch.as_tensor(cams)
        cams = cams.to(device=self.device, dtype=torch.int64)
        if grl_dist.global_heads():
            cams = grl_dist.gather_global(cams)
        b, seq_len = cams.size(0), inputs[0].size(1)
        pairs = cams.view(b // 2, -1)
        self._cam_rows = {'clip': torch.cat((pairs[:, 0], pairs[:, 1])),
                          'frame': cams.unsqueeze(1).expand(b, seq_len).reshape(-1)}
        return super(CameraSEQTrainer, self)._parse_data(inputs)

    def _id_extra(self, rows):
        return {'cams': self._cam_rows[rows]}
