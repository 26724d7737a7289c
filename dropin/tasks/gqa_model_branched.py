from rgqa_amd.tasks.gqa_model_branched import *  # noqa: F401,F403
from rgqa_amd.tasks.gqa_model_branched import GQAModel_branched, MAX_GQA_LENGTH, args  # noqa: F401
