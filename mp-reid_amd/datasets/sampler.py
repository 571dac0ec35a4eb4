"""``RandomIdentitySampler(data_source, batch_size, num_instances)`` with the semantics of the reference's
``datasets/sampler.py:7-66``: a batch is P = batch_size // num_instances identities times K = num_instances images.

``data_source`` is a list of 4-tuples whose second entry is the identity (``(img, pid, camid, viewid)``).  The index lists
are kept per identity in the order the identities first appear.  ``len()`` is the reference's estimate: per identity
``max(n, K)`` images rounded down to a multiple of K.  One pass of ``__iter__`` draws from the GLOBAL ``numpy.random`` and
``random`` generators in the reference's order, so that the same seeds give the same index sequence:

  per identity, in first-appearance order   fewer than K images: ``np.random.choice(idxs, size=K, replace=True)``;
                                            then ``random.shuffle``; then cut into groups of K (a short tail is dropped)
  while at least P identities have groups   ``random.sample`` of P of them, one group of each in the order sampled; an
                                            identity without a group left leaves the pool

No ``torch.utils.data`` base class: ``datasets.make_dataloader.TrainLoader`` only iterates it.
"""
import random

import numpy as np


class RandomIdentitySampler:
    def __init__(self, data_source, batch_size, num_instances):
        if num_instances < 1 or batch_size < num_instances:
            raise ValueError("RandomIdentitySampler: batch_size >= num_instances >= 1")
        self.data_source = data_source
        self.batch_size = batch_size
        self.num_instances = num_instances
        self.num_pids_per_batch = batch_size // num_instances
        self.index_dic = {}                       # pid -> indices, identities in first-appearance order
        for index, item in enumerate(data_source):
            self.index_dic.setdefault(item[1], []).append(index)
        self.pids = list(self.index_dic)
        K = num_instances
        self.length = sum(max(len(v), K) - max(len(v), K) % K for v in self.index_dic.values())

    def __iter__(self):
        K, P = self.num_instances, self.num_pids_per_batch
        groups = {}
        for pid in self.pids:
            idxs = list(self.index_dic[pid])
            if len(idxs) < K:
                idxs = np.random.choice(idxs, size=K, replace=True)
            random.shuffle(idxs)
            groups[pid] = [[idxs[s + j] for j in range(K)] for s in range(0, len(idxs) - K + 1, K)]
        available = list(self.pids)
        order = []
        while len(available) >= P:
            for pid in random.sample(available, P):
                order.extend(groups[pid].pop(0))
                if not groups[pid]:
                    available.remove(pid)
        return iter(order)

    def __len__(self):
        return self.length
