"""robustmvd_amd — MI355X (gfx950) plane-sweep cost-volume engine behind the robustmvd model protocol.

    from robustmvd_amd import create_model
    model = create_model("robust_mvd", pretrained=False, num_gpus=1)
    pred, aux = model.run(images=..., keyview_idx=0, poses=..., intrinsics=...)

The compute path is libmvd_hip.so (robustmvd_amd/csrc, C ABI in include/mvd.h); importing the ops without
the built library raises — there is no CPU fallback.
"""
from .registry import (create_model, prepare_custom_model, register_model, list_models, has_model,  # noqa: F401
                       add_run_function)
from . import models  # noqa: F401  (registers robust_mvd, robust_mvd_5M, mvsnet_train)
from .blocks import (PlanesweepCorrelation, LearnedFusion, CostRegNet, homo_warp, depth_regression,  # noqa: F401
                     compute_sampling_invdepths)
from .models import RobustMVD, MVSNet  # noqa: F401
from .cvp_mvsnet import CVPMVSNet  # noqa: F401  (registers cvp_mvsnet)
from .vis_mvsnet import VisMvsnet  # noqa: F401  (registers vis_mvsnet)
from .ops import sweep_groupcorr_nhwc, soft_argmin, vis_fuse  # noqa: F401
from .serving import FramePipeline, PinnedUploader  # noqa: F401
from .sweep_modes import cvp_proj_cost, vis_cost_volumes, sweep_reduce  # noqa: F401
from . import eval  # noqa: F401,E402
from .eval import create_evaluation, list_evaluations, MultiViewDepthEvaluation  # noqa: F401,E402
from . import depth_fusion  # noqa: F401,E402
from .depth_fusion import DepthFusion, fuse_numpy, merge_numpy, normals_numpy, write_ply  # noqa: F401,E402
from . import cloud_eval  # noqa: F401,E402
from .cloud_eval import (PointCloudEvaluation, CloudScore, evaluate_scene, read_ply, nearest_numpy,  # noqa: F401,E402
                         cloud_scores_numpy, voxel_downsample_numpy)
from . import cloud_register  # noqa: F401,E402
from .cloud_register import register_clouds, register_numpy, Registration  # noqa: F401,E402
from . import cloud_clean  # noqa: F401,E402
from .cloud_clean import (cloud_knn, cloud_neighbourhood, estimate_normals, remove_outliers, cloud_spacing, knn_numpy,  # noqa: F401,E402
                          neighbourhood_numpy, list_moments_numpy, normals_from_moments_numpy, estimate_normals_numpy,
                          remove_outliers_numpy, KNN, Neighbourhood)
from . import tsdf  # noqa: F401,E402
from .mesh import Mesh  # noqa: F401,E402
from .tsdf import TSDFVolume, integrate_numpy, extract_numpy, bounds_from_points  # noqa: F401,E402
from . import render  # noqa: F401,E402
from .render import render_mesh, render_numpy, RenderResult  # noqa: F401,E402
from . import mesh_clean  # noqa: F401,E402
from .mesh_clean import (mesh_components, clean_mesh, vertex_normals, components_numpy, component_table_numpy, clean_numpy,  # noqa: F401,E402
                         vertex_normals_numpy, MeshComponents, CleanResult)
from . import mesh_eval  # noqa: F401,E402
from .mesh_eval import (MeshEvaluation, evaluate_mesh, mesh_distance, sample_mesh, mesh_distance_numpy, mesh_grid_pairs_numpy,  # noqa: F401,E402
                        sample_mesh_numpy)
from . import mesh_simplify  # noqa: F401,E402
from .mesh_simplify import (simplify_mesh, simplify_numpy, cluster_numpy, cluster_quadrics_numpy, place_numpy, SimplifyResult)  # noqa: F401,E402
