from .trainer import SEQTrainer
from .camera import CameraSEQTrainer
from .hybrid import HybridSEQTrainer
from .teacher import (MeanTeacher, MeanTeacherMixin, MeanTeacherSEQTrainer, MeanTeacherHybridSEQTrainer,
                      MeanTeacherCameraSEQTrainer)
from .pseudo import (PseudoLabels, ProxyLabels, HybridLabels, SelfPacedState, pseudo_labels, self_paced_labels,
                     train_unsupervised)
