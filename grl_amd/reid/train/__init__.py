from .trainer import SEQTrainer
from .camera import CameraSEQTrainer
from .hybrid import HybridSEQTrainer
from .teacher import MeanTeacher, MeanTeacherSEQTrainer
from .pseudo import (PseudoLabels, ProxyLabels, HybridLabels, SelfPacedState, pseudo_labels, self_paced_labels,
                     train_unsupervised)
