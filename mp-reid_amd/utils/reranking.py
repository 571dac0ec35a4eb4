"""Drop-in for the reference's ``utils/reranking.py`` (k-reciprocal re-ranking, Zhong et al. CVPR'17),
computed on the MI355X through libmpreid_hip.so.

Same call as the reference (utils/reranking.py:29):

    re_ranking(probFea, galFea, k1, k2, lambda_value, local_distmat=None, only_local=False)
        -> np.ndarray float32 [num_query, num_gallery]

probFea / galFea are torch tensors (any device); local_distmat an optional (nq+ng) x (nq+ng) array.
The algorithm and every fp16/fp32 rounding point follow the reference (see csrc/rerank.h and the rerank_*.hip files); the
dense N x N float16 ``V`` of the reference is replaced by sparse rows, which changes no result.

Any k1 >= 0 / k2 >= 1 is answered, as by the reference: the fast algorithms have two limits (include/mpreid.h
"Limits"); a call outside them runs mpreid.ops.RERANK_WIDE instead -- the same bits, slower.  Every call inside
the limits takes the path it always took.
"""
import numpy as np
import torch

from mpreid import ops as _ops


def _default_algo(probFea, galFea, k1, k2, local_distmat):
    """RERANK_AUTO when it accepts the problem, RERANK_WIDE otherwise (asked beforehand: a refused call would leave an error
    string behind and cost a workspace allocation)"""
    nq, ng, d = int(probFea.shape[0]), int(galFea.shape[0]), int(probFea.shape[1])
    if _ops.rerank_fits(nq, ng, d, k1, k2, local_distmat is not None, _ops.RERANK_AUTO):
        return _ops.RERANK_AUTO
    return _ops.RERANK_WIDE


def re_ranking_device(probFea, galFea, k1, k2, lambda_value, local_distmat=None, only_local=False, timing=False,
                      algo=None):
    """Same computation, result left on the GPU; returns (tensor [nq, ng], stats dict).  algo: None (the default:
    mpreid.ops.RERANK_AUTO -- bit-parity -- where it applies, RERANK_WIDE for k1 / k2 beyond its limits), or one of
    mpreid.ops.RERANK_AUTO ... RERANK_SPARSE_SPLIT3 (blend-term distances from the fp16 matrix cores, outputs within
    1e-6, ranks identical; the large-N option), RERANK_WIDE, honoured as given."""
    if algo is None:
        algo = _default_algo(probFea, galFea, k1, k2, local_distmat)
    return _ops.re_ranking(probFea, galFea, k1, k2, lambda_value, local_distmat=local_distmat,
                           only_local=only_local, timing=timing, algo=algo)


def re_ranking(probFea, galFea, k1, k2, lambda_value, local_distmat=None, only_local=False):
    if isinstance(probFea, np.ndarray):
        probFea = torch.from_numpy(probFea)
    if isinstance(galFea, np.ndarray):
        galFea = torch.from_numpy(galFea)
    final_dist, _ = re_ranking_device(probFea, galFea, k1, k2, lambda_value, local_distmat, only_local)
    return final_dist.cpu().numpy()
