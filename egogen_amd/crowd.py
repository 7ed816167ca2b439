"""The people of one call of `generate_sequence_to_goal` who see each other: `PersonGroups`, the partition of the b sequences into
groups that the joint step of the greedy search (entry egx_primitive_select_joint, csrc/genop_joint.hip) reads as CSR tensors on
the device.  A group is the people who share a scene and a time line; within a group every member chooses its next primitive
against the others' current choices."""
from __future__ import annotations

import numpy as np
import torch

MAX_GROUP = 32          # EGX_MAX_GROUP of include/egogen_hip.h
MAX_SWEEPS = 8          # EGX_MAX_SWEEPS
PAIR_MODELS = ("cylinder", "markers")       # what a person is to the joint step: a cylinder round the pelvis, or the 67 blended markers
PAIR_TABLE_CAP_BYTES = 1 << 30              # the marker model's distance table (pairs x N x N x 18 float32) may take this much, no more


class PersonGroups:
    """ids [b] the group of every sequence as given; start [G+1] / member [b] the CSR form: group g holds the sequences
    member[start[g]:start[g+1]] in ascending order, the groups in order of first appearance.  Built on the host (`from_ids`, no
    device needed); `to(device)` makes the int32 tensors `group_start` / `group_member` the kernel reads, `member_group` [b], the
    group of every sequence, and `pair_start` [G+1], the first unordered pair of members of every group (the cumulative sum of
    P (P - 1) / 2: the layout of egx_crowd_metrics and of the marker model's distance table)."""

    def __init__(self, ids, start, member):
        self.ids, self.start, self.member = ids, start, member
        self.device = self.group_start = self.group_member = self.member_group = self.pair_start = None

    def __len__(self):
        return len(self.start) - 1

    @property
    def sizes(self):
        return np.diff(self.start)

    @property
    def pair_offsets(self):
        """[G+1] int64 on the host: pair_start; its last entry is the number of unordered pairs of members"""
        sizes = self.sizes.astype(np.int64)
        return np.concatenate([[0], np.cumsum(sizes * (sizes - 1) // 2)])

    def pair_table_bytes(self, n_candidates: int) -> int:
        """bytes of the marker model's distance table [pairs, N, N, 18] float32"""
        return int(self.pair_offsets[-1]) * int(n_candidates) ** 2 * 18 * 4

    @classmethod
    def from_ids(cls, groups, b: int) -> "PersonGroups":
        """groups: [b] integers; sequences with equal ids are one group.  ValueError for another length, values that are no
        integers, or a group of more than 32 members."""
        if torch.is_tensor(groups):
            groups = groups.detach().cpu().numpy()
        g = np.asarray(groups)
        if g.ndim != 1 or g.shape[0] != int(b):
            raise ValueError(f"groups must hold {int(b)} ids, one per sequence, got shape {tuple(g.shape)}")
        if g.dtype == bool or not (np.issubdtype(g.dtype, np.integer) or
                                   (np.issubdtype(g.dtype, np.floating) and np.isfinite(g).all() and (g == np.round(g)).all())):
            raise ValueError(f"groups must be integers, got {g.dtype}: {g.tolist()}")
        g = g.astype(np.int64)
        order, members = [], {}
        for i, v in enumerate(g.tolist()):
            if v not in members:
                members[v] = []
                order.append(v)
            members[v].append(i)
        for v in order:
            if len(members[v]) > MAX_GROUP:
                raise ValueError(f"group {v} has {len(members[v])} members, at most {MAX_GROUP} people can see each other")
        start = np.cumsum([0] + [len(members[v]) for v in order]).astype(np.int32)
        member = np.asarray([i for v in order for i in members[v]], np.int32)
        return cls(g, start, member)

    def to(self, device) -> "PersonGroups":
        device = torch.device(device)
        self.group_start = torch.from_numpy(self.start).to(device)
        self.group_member = torch.from_numpy(self.member).to(device)
        # the inverse of the CSR, [b] int32: the group of every sequence (what egx_primitive_observe_people finds a sequence's mates by)
        of = np.zeros(len(self.member), np.int32)
        of[self.member] = np.repeat(np.arange(len(self), dtype=np.int32), self.sizes)
        self.member_group = torch.from_numpy(of).to(device)
        self.pair_start = torch.from_numpy(self.pair_offsets.astype(np.int32)).to(device)
        self.device = device
        return self
