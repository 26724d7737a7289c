from rgqa_amd.tasks.gqa_branched_layer import *  # noqa: F401,F403
from rgqa_amd.tasks.gqa_branched_layer import GQAModel_branched, GQAProjector, MAX_GQA_LENGTH, args  # noqa: F401
