"""Worker of tests/test_gpu_point_loss.py::test_two_ranks_with_shared_statistics_equal_one_rank_with_the_batch: rank r trains on cloud r of a
WORLD_SIZE-cloud batch under Trainer(loss=<kind>) with statistics shared over the process group (gloo here: all ranks use the same GPU), and
writes its loss, accuracy, logits, the averaged gradient buffer and the step's collective counts to <out>.rank<r>.npz -- then the counts of
the same step under the cross-entropy, and of the Dice step with per-GPU statistics."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import torch
    import torch.distributed as dist
    import test_gpu_train as T
    out, kind = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, xyz, feats = T.syncbn_case(world)
    labels = T.syncbn_labels(cfg, xyz)[rank:rank + 1]
    d_feats, d_lab = torch.from_numpy(feats[rank:rank + 1]).cuda(), torch.from_numpy(labels).cuda()

    def step(loss, sync_bn):
        tr, pyr, _, _, _, _ = T._setup(cfg, xyz[rank:rank + 1], feats[rank:rank + 1], labels=labels, sync_bn=sync_bn, oracle_pyramid=False, loss=loss)
        value = tr.train_step(pyr, d_feats, d_lab, dist=dist)
        torch.cuda.synchronize()
        res = dict(loss=float(value), accuracy=float(tr.last_accuracy), logits=tr.last_logits.cpu().numpy(), grad=tr.grad.cpu().numpy(),
                   flat=tr.flat.cpu().numpy(), stats=tr.collective_stats())
        tr.close()
        return res

    shared = step(kind, True)
    ce = step("ce", True)
    local = step(kind, False)
    np.savez(out + ".rank%d.npz" % rank, loss=shared["loss"], accuracy=shared["accuracy"], logits=shared["logits"], grad=shared["grad"], flat=shared["flat"],
             calls_dice=shared["stats"]["calls"], bytes_dice=shared["stats"]["bytes"], calls_ce=ce["stats"]["calls"], bytes_ce=ce["stats"]["bytes"],
             calls_local=local["stats"]["calls"], bytes_local=local["stats"]["bytes"])
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
