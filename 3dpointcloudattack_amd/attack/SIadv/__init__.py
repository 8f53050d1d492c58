"""attack/SIadv of the reference: the shape-invariant white-box attack (SIadv_attack.py: PointCloudAttack with
``ifgm_ours``, batched, the normals re-estimated on the device) and the pre-processing defences it is run against
(baselines/defense: drop_points, DUP_Net). The three query attacks of SIadv_attack.py (simba, simbapp, ours) are out of
scope."""
