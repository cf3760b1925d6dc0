"""``ICPLosses``: the reference's list-based loss module (src/losses/icp_losses.py:10-158).

The training step does not go through this class (it uses the fused image-based kernels of
delora_amd.geometry); it exists so that code written against the reference's list interface keeps working:
correspondences come from the exact HIP tree search over the target list (``geometry.PointTree``, the counterpart of the
reference's cKDTree; small lists stay on the quadratic kernel, which returns the same indices), the loss arithmetic on the
gathered pairs is a handful of torch ops so that gradients flow into the (already transformed) inputs as they do in
the reference."""
import torch

from .. import geometry


class ICPLosses(torch.nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        if config["normal_loss"] not in ("squared", "linear"):
            raise Exception("The normal loss which is defined here is not admissible.")

    _warned_quadratic = False
    # Source points x target points from which a search goes through the tree.  Read off profiles/nn_list_bench.json (one MI355X,
    # Ms = Mt = n, build + query against the exhaustive kernel, ms per call over the four pose regimes): n = 8 192: 0.40-0.53
    # against 0.33, the exhaustive kernel still wins; n = 32 768: 0.44-0.71 against 1.34, the tree wins in every regime
    # (131 072: 0.72-1.37 against 8.0).  The crossover is the smallest measured size at which the tree wins everywhere.
    tree_min_pairs = 32768 * 32768

    @staticmethod
    def _wants_tree(n_src, n_tgt):
        return n_src * n_tgt >= ICPLosses.tree_min_pairs

    @staticmethod
    def find_target_correspondences(target_point_cloud, source_point_cloud, tree=None):
        """Index of the exact nearest target point for every source point (both ``[1,3,M]``): tree search (``geometry.PointTree``,
        built here unless the caller passes the one it already holds for this target list), or the exhaustive kernel for lists too
        small for the tree to pay.  Both give the same indices.  Only a call that really goes the quadratic way above 32 k points
        says so, once."""
        n_src, n_tgt = int(source_point_cloud.shape[-1]), int(target_point_cloud.shape[-1])
        if tree is None and ICPLosses._wants_tree(n_src, n_tgt):
            tree = geometry.PointTree(target_point_cloud[0])
        if tree is not None:
            return tree.query(source_point_cloud[0]).long()
        if max(n_src, n_tgt) > 32768 and not ICPLosses._warned_quadratic:
            ICPLosses._warned_quadratic = True
            import warnings
            warnings.warn(f"ICPLosses (list interface): exhaustive nearest-neighbour search over {n_src} x {n_tgt} points "
                          f"({n_src * n_tgt / 1e9:.1f} G distance evaluations per call); the image-based step path "
                          "(Deployer.step / geometry.nn_correspond) is exact as well and ~100x faster", RuntimeWarning, stacklevel=3)
        return geometry.nn_bruteforce(source_point_cloud[0], target_point_cloud[0]).long()

    def forward(self, source_point_cloud_transformed, source_normal_list_transformed, target_point_cloud,
                target_normal_list, compute_pointwise_loss_bool):
        cfg = self.config
        dev = target_point_cloud.device
        zero = torch.zeros(1, device=dev)
        losses = {"loss_po2po": zero, "loss_po2pl": zero, "loss_po2pl_pointwise": zero, "loss_pl2pl": zero}
        if cfg["po2po_alone"]:                                             # icp_losses.py:36-45
            if cfg["point_to_plane_loss"] or cfg["plane_to_plane_loss"]:       # the reference dies here (:135-146)
                raise Exception("po2po_alone needs point_to_plane_loss and plane_to_plane_loss switched off.")
            nn = self.find_target_correspondences(target_point_cloud, source_point_cloud_transformed)     # builds its own tree
            if cfg["point_to_point_loss"]:
                d = source_point_cloud_transformed - target_point_cloud[:, :, nn]
                losses["loss_po2po"] = (d * d).mean()
            return losses, None
        s_has = (source_normal_list_transformed[0] != 0).any(dim=0)          # :48-50
        t_has = (target_normal_list[0] != 0).any(dim=0)                      # :51-52
        src_w = source_point_cloud_transformed[:, :, s_has]
        srcn_w = source_normal_list_transformed[:, :, s_has]
        # ONE tree per call, shared by both searches (decided on the whole source list: the two searches split it between them)
        n_tgt = int(target_point_cloud.shape[-1])
        tree = (geometry.PointTree(target_point_cloud[0])
                if self._wants_tree(int(source_point_cloud_transformed.shape[-1]), n_tgt) else None)
        nn_w = self.find_target_correspondences(target_point_cloud, src_w, tree)
        if cfg["point_to_point_loss"]:                                     # :85-100: neither side has a normal
            src_wo = source_point_cloud_transformed[:, :, ~s_has]
            nn_wo = self.find_target_correspondences(target_point_cloud, src_wo, tree)
            keep = ~t_has[nn_wo]
            d = src_wo[:, :, keep] - target_point_cloud[:, :, nn_wo[keep]]
            losses["loss_po2po"] = (d * d).mean()
        keep = t_has[nn_w]                                                 # :110-121: target must have a normal too
        s_k, sn_k = src_w[:, :, keep], srcn_w[:, :, keep]
        t_k, tn_k = target_point_cloud[:, :, nn_w[keep]], target_normal_list[:, :, nn_w[keep]]
        if cfg["point_to_plane_loss"]:                                     # :196-203
            dvec = s_k - t_k
            r = (dvec * tn_k).sum(dim=1)
            losses["loss_po2pl"] = (r * r).mean()
            if compute_pointwise_loss_bool:
                losses["loss_po2pl_pointwise"] = dvec
        if cfg["plane_to_plane_loss"]:                                     # :224-238
            if cfg["normal_loss"] == "linear":
                c = (sn_k * tn_k).sum(dim=1)
                losses["loss_pl2pl"] = ((1 - c) ** 2).mean()
            else:
                e = sn_k - tn_k
                losses["loss_pl2pl"] = (e * e).sum(dim=1).mean()
        plotting = {"scan_2_transformed": s_k, "normals_2_transformed": sn_k}
        return losses, plotting
