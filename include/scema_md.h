/*
 * scema_md.h -- C ABI of the MI355X-native microscale stress-evaluation engine that drops into
 * SCEMa's STMDProblem / STMDSync path.
 *
 * Plain C: pointers and sizes only, no torch / HIP / C++ types.  Each entry point names the
 * reference interface it replaces (paths relative to the SCEMa tree).
 *
 * Tensor conventions (reference): rank-2 symmetric tensors travel as 6 doubles in deal.II raw
 * order xx,yy,zz,xy,xz,yz (headers/scale_bridging_data.h:12-19, FE_problem.h:1344-1346); rank-4
 * stiffness as 36 doubles in init.*.stiff file order (headers/read_write.h:149-171).
 */
#ifndef SCEMA_MD_H
#define SCEMA_MD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCEMA_MD_OK 0
#define SCEMA_MD_ERR_ARG 1        /* bad argument / unknown force field (stmd_problem.h:462-467) */
#define SCEMA_MD_ERR_NOSTATE 2    /* required replica / state missing (stmd_problem.h:125-132 asserts) */
#define SCEMA_MD_ERR_DEVICE 3     /* HIP runtime failure */
#define SCEMA_MD_ERR_BOX 4        /* box smaller than 2*(cutoff+skin) */
#define SCEMA_MD_ERR_IO 5
#define SCEMA_MD_ERR_OVERFLOW 6   /* neighbour capacity exceeded even after regrowth */

#define SCEMA_MD_NPART 8          /* lj, coul, bond, angle, dihedral, improper, kspace, shake */
#define SCEMA_MD_QP_NONE ((int32_t)0xFFFFFFFF) /* most_recent_qp_id "none": uint32 max as int, stmd_problem.h:126 */

typedef struct scema_md_engine scema_md_engine;

/* Run-level settings = what the reference's LAMMPS scripts fix for the OPLS path
 * (lammps_scripts_opls/in.set.lammps:27-40, in.strain.lammps:71,80). */
typedef struct {
  double cut_lj;           /* 12.0  pair_style lj/cut/coul/long 12.0 9.0 */
  double cut_coul;         /*  9.0 */
  double skin;             /*  2.0  neighbor 2.0 bin */
  int32_t neigh_delay;     /*  5    neigh_modify every 1 delay 5 check yes */
  double kspace_accuracy;  /* 1e-4  kspace_style pppm 0.0001 (sets g_ewald; reciprocal sum: see kspace_style) */
  double shake_tol;        /* 1e-3  fix shake 0.001 20 1000 m 1.0 */
  int32_t shake_maxiter;   /* 20 */
  double shake_mass;       /* 1.0 ; <= 0 disables SHAKE */
  double t_period;         /* 100.0 fix nvt temp T T 100.0 */
  int32_t t_chain;         /* 3 */
  int32_t device;          /* HIP device ordinal */
  int32_t max_batch;       /* simulations advanced together per launch group; 0 = all that fit */
  int32_t profile;         /* !=0: HIP-event timing of every pair-kernel launch (scema_md_get_profile) */
  int32_t kspace_style;    /* 1 (default): PPPM as `kspace_style pppm 0.0001` asks for (in.set.lammps:36; order 5, ik differentiation,
                            * hipFFT; grid and g_ewald by the rules of pppm.cpp as restated in scema_amd/csrc/engine/engine_kspace.cpp / oracle/md_oracle.c;
                            * DESIGN.md 5c); 0: the reciprocal part as the plain Ewald sum PPPM approximates, at kspace_accuracy
                            * (LAMMPS' initial g_ewald estimate, k-vectors by the RMS criterion of kspace_style ewald) */
} scema_md_params;

void scema_md_default_params(scema_md_params *p);

/* Content of one equilibrated replica = what init.<mat>_<rep>.bin carries in the reference
 * (stmd_problem.h:99-100, stmd_sync.h:388).  0-based atom and type indices; angles in radians;
 * eps/sigma are ntypes x ntypes (already mixed).  box = xlo,ylo,zlo,xhi,yhi,zhi,xy,xz,yz. */
typedef struct {
  int32_t natoms, ntypes;
  const int32_t *type;
  const double *charge;
  const double *mass;      /* per type */
  const double *eps, *sigma;
  int32_t nbonds, nbondtypes;
  const int32_t *bond_atoms, *bond_type;
  const double *bond_coeff;      /* K, r0 */
  int32_t nangles, nangletypes;
  const int32_t *angle_atoms, *angle_type;
  const double *angle_coeff;     /* K, theta0 */
  int32_t ndihedrals, ndihedraltypes;
  const int32_t *dihedral_atoms, *dihedral_type;
  const double *dihedral_coeff;  /* K1..K4 (dihedral_style opls) */
  int32_t nimpropers, nimpropertypes;
  const int32_t *improper_atoms, *improper_type;
  const double *improper_coeff;  /* K, chi0 */
  double special_lj[3], special_coul[3]; /* in.init.lammps:31 -> 0 0 1 */
  double box[9];
  const double *x, *v;           /* [natoms*3] */
} scema_md_system;

/* Mirrors HMM::MDSim<3> (headers/md_sim.h:15-58). */
typedef struct {
  int32_t qp_id, most_recent_qp_id, replica /* 1-based */, material;
  const char *matid, *time_id, *output_folder, *restart_folder, *scripts_folder, *log_file, *force_field;
  double strain[6];      /* IN  raw order; Angstrom (strain x init_length, stmd_sync.h:552-557) */
  double stiffness[36];  /* IN  Hooke mode only, file order */
  double timestep_length, temperature, strain_rate;
  int32_t nsteps_sample;
  int32_t output_homog, checkpoint;
  double stress[6];      /* OUT Pa, raw order: -<P> * 101325 (stmd_problem.h:335-341) */
  int32_t stress_updated;/* OUT */
} scema_mdsim;

/* ---- engine lifetime ---- */
int scema_md_create(const scema_md_params *p, scema_md_engine **out);
void scema_md_destroy(scema_md_engine *e);
const char *scema_md_last_error(const scema_md_engine *e);

/* ---- replica registry: replaces "read_restart init.<mat>_<rep>.bin" (stmd_problem.h:204) ---- */
int scema_md_register_replica(scema_md_engine *e, const char *matid, int32_t replica, const scema_md_system *sys);
/* atoms of a registered replica, 0 if (matid, replica) is not registered */
int32_t scema_md_replica_natoms(scema_md_engine *e, const char *matid, int32_t replica);
/* reads a replica file written by scema_md_write_replica_file (our container for init.*.bin) */
int scema_md_load_replica_file(scema_md_engine *e, const char *matid, int32_t replica, const char *path);
int scema_md_write_replica_file(const char *path, const scema_md_system *sys);
/* a registered replica with its current initial state (e.g. after scema_md_equilibrate) as such a file: what
 * `write_restart init.<mat>_<rep>.bin` keeps in the reference (init_material_problem.h:208-210) */
int scema_md_save_replica_file(scema_md_engine *e, const char *matid, int32_t replica, const char *path);
/* LAMMPS text data file of atom_style full (`write_data` of a replica equilibrated with the reference's
 * in.init.lammps): register it directly, or convert it to the replica container.  special_bonds weights are
 * not stored in data files; NULL means the reference's "lj/coul 0 0 1" (in.init.lammps:31). */
int scema_md_load_lammps_data(scema_md_engine *e, const char *matid, int32_t replica, const char *path,
                              const double special_lj[3], const double special_coul[3]);
int scema_md_convert_lammps_data(const char *data_path, const char *replica_path, const double special_lj[3],
                                 const double special_coul[3]);

/* LAMMPS binary restart files in the layout of the version the reference pins (LAMMPS 17Nov16, reference README.md:31-37):
 * the `init.<mat>_<rep>.bin` that stmd_problem.h:204 reads and the `last.*` / `lcts.*` states that stmd_problem.h:258,268
 * write.  probe: header of any restart file.  read_atoms: tag, type, image flags (3 per atom), wrapped x, v in file order
 * (atom_style atomic or full; NULL outputs are skipped).  load / convert: atom_style full + pair lj/cut/coul/long +
 * bond/angle harmonic + dihedral opls + improper harmonic, units real -> replica (compare info.cut_lj / cut_coul with the
 * engine's parameters: the engine takes its cutoffs from scema_md_params).  write: one-process restart of a replica in
 * the same layout. */
typedef struct {
  char version[32], units[16], atom_style[32], pair_style[64];
  int64_t natoms, ntimestep, nbonds, nangles, ndihedrals, nimpropers;
  int32_t ntypes, nbondtypes, nangletypes, ndihedraltypes, nimpropertypes, triclinic, nprocs, reserved;
  double box[9];            /* xlo,ylo,zlo,xhi,yhi,zhi,xy,xz,yz */
  double timestep;
  double special_lj[3], special_coul[3];
  double cut_lj, cut_coul;  /* pair lj/cut/coul/long settings, 0 if the file has no such block */
  double mass[16];          /* first 16 types */
  char error[160];
} scema_lammps_restart_info;
int scema_md_probe_lammps_restart(const char *path, scema_lammps_restart_info *info);
int scema_md_read_lammps_restart_atoms(const char *path, int64_t capacity, int64_t *tag, int32_t *type, int32_t *image,
                                       double *x, double *v);
/* load: an atom_style full restart of the OPLS styles, or an atom_style atomic one (units real or metal: the reference's
 * examples/streched_polyhedron/nanoscale_input/init.sic_1.bin), which registers a BARE replica -- types, masses, box, positions,
 * velocities (A/ps -> A/fs for units metal); no charges, no topology, zero Lennard-Jones coefficients -- for a potential attached to the
 * material id with scema_md_sw_configure.  convert takes atom_style full files only. */
int scema_md_load_lammps_restart(scema_md_engine *e, const char *matid, int32_t replica, const char *path);
int scema_md_convert_lammps_restart(const char *restart_path, const char *replica_path);
int scema_md_write_lammps_restart(const char *path, const scema_md_system *sys, double cut_lj, double cut_coul,
                                  double timestep, int64_t ntimestep);

/* ---- the hot path ---- */
/* Replaces STMDProblem<3>::strain (stmd_problem.h:458-496) for the whole vector that
 * STMDSync::execute_inside_md_simulations iterates (stmd_sync.h:570-618).  Every rank passes the SAME vector.
 * Which rank runs simulation i is decided by the planner of scema_amd/csrc/host/sim_plan.h (identical on every rank):
 * a fresh balanced batch gives the reference's round robin i % world (stmd_sync.h:583); afterwards a simulation runs
 * where the state it continues from lives (a state is resident in ONE GPU's HBM, the update_list changes from step to
 * step, FE_problem.h:1330-1350), and ragged batches are levelled by MD steps (nts + nss).
 * State branch rule of stmd_problem.h:116-138,185-207: load from most_recent_qp_id if != qp_id, else qp_id, else the
 * registered init state; always store under qp_id.  hooke != 0: sigma = C:eps (stmd_problem.h:479-483).
 *   - no communicator attached (world may still be > 1): only this rank's share is evaluated, the others are left
 *     untouched (stress_updated = 0) and the caller gathers (scema_md_copy_local_stress + scema_md_scatter_gathered:
 *     the result buffer carries this rank's status word, so the caller enters its collective even after a failed call);
 *     a request whose source state lives on another rank is an error (SCEMA_MD_ERR_NOSTATE);
 *   - communicator attached (scema_md_comm_init_*): the call is collective -- the ranks first agree (a 16-byte
 *     handshake per rank: status of the local pre-checks + hash of the plan each rank computed; a mismatch is an error
 *     on every rank instead of a hang), states that have to change GPU travel, then ONE all-gather returns every stress
 *     to every rank (replaces STMDSync::share_stresses, stmd_sync.h:620-726): on return every sims[i].stress is set on
 *     every rank.  The all-gather carries a status word per rank: a share that failed on one rank (list overflow after
 *     regrowth, a replica that blew up, a missing state) makes the call fail on EVERY rank, none is left waiting.
 * Requests are validated on every rank before anything is planned, so a bad request is refused by all ranks alike.
 * A failed call leaves the state store and the owner directory as it found them -- ON EVERY RANK when a communicator is
 * attached (the ranks learn of each other's failure inside the call and all roll back): states that had already been
 * advanced are put back from their backups (the reference stops the whole run at this point, exit(1)).  Without a
 * communicator a rank whose own share succeeded learns of another rank's failure only in the caller's collective: its share
 * waits for that (scema_md_settle_update below) and is taken back there.
 * What the ranks must share for their plans to agree: the same replicas registered, the same request vectors, and every
 * call that edits the state store (set_state, drop_state, load_state_file, equilibrate) made on every rank. */
int scema_md_strain_batch(scema_md_engine *e, scema_mdsim *sims, int32_t n_sims, int32_t hooke,
                          int32_t rank, int32_t world);
/* literal per-simulation drop-in */
int scema_md_strain(scema_md_engine *e, scema_mdsim *sim, int32_t hooke);

/* ---- multi-GPU: one process per GPU, the engine owns the collective ----
 * RCCL over xGMI: rank 0 calls scema_md_comm_unique_id and the host program broadcasts the 128 bytes (MPI_Bcast in
 * SCEMa, any store elsewhere); every rank then calls scema_md_comm_init_rccl (ncclCommInitRank on the engine's
 * device).  Replaces the MPI traffic of stmd_sync.h:620-726 (per-simulation MPI_Isend/Recv of 6 doubles) by one
 * ncclAllGather per update, and the shared-file-system hand-over of last.<qp>.* states by ncclSend/ncclRecv. */
#define SCEMA_MD_COMM_ID_BYTES 128
int scema_md_comm_unique_id(void *id /* [SCEMA_MD_COMM_ID_BYTES] */);
int scema_md_comm_init_rccl(scema_md_engine *e, const void *id, int32_t rank, int32_t world);
/* Host transport instead (MPI of the host program; gloo in the CPU tests): buffers are host memory.
 * allgather: every rank contributes bytes_per_rank bytes, recv holds world * bytes_per_rank.  send/recv: blocking
 * point-to-point (may be NULL if states never have to move).  Return 0 on success. */
typedef int (*scema_md_host_allgather_fn)(void *ctx, const void *send, void *recv, int64_t bytes_per_rank);
typedef int (*scema_md_host_send_fn)(void *ctx, const void *buf, int64_t bytes, int32_t dst_rank);
typedef int (*scema_md_host_recv_fn)(void *ctx, void *buf, int64_t bytes, int32_t src_rank);
int scema_md_comm_init_host(scema_md_engine *e, int32_t rank, int32_t world, scema_md_host_allgather_fn allgather,
                            scema_md_host_send_fn send, scema_md_host_recv_fn recv, void *ctx);
void scema_md_comm_destroy(scema_md_engine *e);
int32_t scema_md_comm_world(const scema_md_engine *e);   /* 1 = no communicator */
int32_t scema_md_comm_rank(const scema_md_engine *e);
int scema_md_comm_stats(const scema_md_engine *e, int64_t *allgathers, int64_t *migrations);
int64_t scema_md_comm_handshakes(const scema_md_engine *e);   /* agreement handshakes so far (one per update when world > 1) */
/* rank recorded as the owner of a stored state, -1 = none recorded (held wherever it was set) */
int32_t scema_md_state_owner(const scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica);

/* Plan of the last scema_md_strain_batch: owner[i] = rank that ran simulation i, pos[i] = its slot in that rank's
 * result buffer, cap = slots per rank. */
int scema_md_last_plan(const scema_md_engine *e, int32_t n_sims, int32_t *owner, int32_t *pos, int32_t *cap);
/* Device-side result buffer of the last scema_md_strain_batch: 6*max(cap,1) doubles in HBM, simulation i of this rank
 * at offset 6*pos[i], followed by SCEMA_MD_RESULT_TRAILER words: the status of this rank's share (0, or the error code
 * scema_md_strain_batch returned) and the hash of the plan this rank computed.  The operand of the all-gather when the
 * caller runs the collective itself: scema_md_local_result_doubles() doubles per rank. */
#define SCEMA_MD_RESULT_TRAILER 2
void *scema_md_local_stress_device_ptr(scema_md_engine *e);
int32_t scema_md_local_stress_count(const scema_md_engine *e);   /* = cap */
int32_t scema_md_local_result_doubles(const scema_md_engine *e); /* = 6*max(cap,1) + SCEMA_MD_RESULT_TRAILER */
/* copy that buffer (all scema_md_local_result_doubles() of it) into caller memory (a device pointer, e.g. the send
 * buffer of the all-gather, or host) */
int scema_md_copy_local_stress(scema_md_engine *e, void *dst, int32_t dst_on_device);
/* after the caller's all-gather into gathered[world][scema_md_local_result_doubles()] (host memory): check every
 * rank's status word and plan hash (an error here is an error on every rank), then fill sims[i].stress /
 * stress_updated for every i by the plan of the last scema_md_strain_batch (rank-0 bookkeeping of stmd_sync.h:698-725) */
int scema_md_scatter_gathered(scema_md_engine *e, const double *gathered, scema_mdsim *sims, int32_t n_sims);
/* Without a communicator an update of a world of several ranks WAITS after scema_md_strain_batch (backups kept, owner directory
 * uncommitted) until the caller's collective has shown every rank's status word: scema_md_scatter_gathered settles it (an error
 * there takes this rank's share back too); a host that scatters the gathered buffer itself calls this with failed != 0 / 0.  The
 * next scema_md_strain_batch lets an unsettled update stand. */
int scema_md_settle_update(scema_md_engine *e, int32_t failed);
/* How many updates the NEXT call found unsettled and let stand (world > 1, no communicator attached, neither scema_md_scatter_gathered nor
 * scema_md_settle_update called in between): 0 in a host that follows the protocol; a warning is printed the first time. */
int64_t scema_md_unsettled_updates(const scema_md_engine *e);

/* The planner alone (scema_amd/csrc/host/sim_plan.h; pure host arithmetic, no GPU): owner/pos/cap as above, moves =
 * (simulation, from, to) triples of the states that would travel; cost NULL = equal cost; commit != 0 records the
 * owners for the next call, as a successful scema_md_strain_batch does. */
typedef struct scema_plan_dir scema_plan_dir;
scema_plan_dir *scema_plan_dir_create(void);
void scema_plan_dir_destroy(scema_plan_dir *d);
int scema_plan_update(scema_plan_dir *d, const scema_mdsim *sims, int32_t n_sims, const double *cost, int32_t world,
                      int32_t *owner, int32_t *pos, int32_t *cap, int32_t *moves /* 3 per move, room for n_sims */,
                      int32_t *n_moves, int32_t commit);

/* ---- persistent per-(qp,mat,replica) state: replaces last.<qp>.<mat>_<rep>.dump / lcts.* files
 * (stmd_problem.h:108-138,257-273; stmd_sync.h:167-187) ---- */
int scema_md_has_state(const scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica);
int scema_md_get_state(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica,
                       double box[9], double *x, double *v);
int scema_md_set_state(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica,
                       const double box[9], const double *x, const double *v);
int scema_md_drop_state(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica);
int scema_md_save_state_file(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, const char *path);
/* load: the engine's own state container, or a LAMMPS 17Nov16 binary restart of the same replica as the reference writes
 * last.<qp>.* / lcts.<qp>.* (told apart by the magic string; atoms matched by tag, unwrapped with the image flags) */
int scema_md_load_state_file(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, const char *path);
/* the state as a LAMMPS 17Nov16 binary restart (what stmd_problem.h:258,268 write), for hand-over to a LAMMPS-based run */
int scema_md_save_state_lammps(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, const char *path,
                               double timestep, int64_t ntimestep);

/* the state as a LAMMPS text dump `id type xs ys zs vx vy vz ix iy iz` (what the reax branch of the reference writes as
 * last.<qp>.* / lcts.<qp>.*, stmd_problem.h:261-264,270-272, and re-reads with `rerun ... dump x y z vx vy vz ix iy iz box yes
 * scaled yes`, :190-194); read back by scema_md_load_state_file.  precise 0: LAMMPS' default "%g" columns (six digits, what the
 * reference's files hold); != 0: 17 digits (exact round trip). */
int scema_md_save_state_dump(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, const char *path,
                             int64_t ntimestep, int32_t precise);

/* ---- init_material: the quantities EQMDProblem::lammps_equilibration derives from an equilibrated
 * replica (init_material_problem.h:196-300): box lengths, initial stress (ELASTIC/in.homogenization.lammps: NVT + SHAKE
 * sampling) and the stiffness tensor by +-strain_ampl finite strains in the six directions (ELASTIC/in.modulus.lammps,
 * bi-displace.mod.lammps: fix deform ... delta over nsstrain steps, then nsteps_sample steps of sampling, fix nvt only).
 * The 13 runs are one batch on the GPU.  The equilibration schedule itself (in.init.lammps: minimise, heat, cool) is not
 * part of this call (scema_md_equilibrate below is): the registered replica is taken as the equilibrated state ("Reuse of
 * state data", :175-184).  With a ReaxFF force field selected (scema_md_reax_configure / scema_md_reax_activate) both calls run on
 * the ReaxFF force stage.
 * length[3]; stress[6] in Pa, file order 00,01,02,11,12,22; stiff[36] in Pa, file order of init.*.stiff. */
typedef struct {
  double timestep_length;  /* fs   "molecular dynamics parameters.timestep length" */
  double temperature;      /* K */
  int32_t nsteps_sample;   /* nssample0 = nssample */
  double strain_ampl;      /* "up": strain perturbation amplitude */
  double strain_rate;      /* 1/fs: nsstrain = ceil(up/(dt*rate)/10)*10 (init_material_problem.h:226) */
} scema_md_eqparams;
int scema_md_init_material(scema_md_engine *e, const char *matid, int32_t replica, const scema_md_eqparams *p,
                           double length[3], double stress[6], double stiff[36]);

/* ---- init_material, first part: the equilibration schedule EQMDProblem::lammps_equilibration runs when no state exists yet
 * (init_material_problem.h:167-174: in.init.lammps).  What lammps_scripts_opls/in.init.lammps:44-215 prescribes, on the GPU:
 * velocity create 200 K, min_style sd + minimize 1e-7 1e-11 nsinit 50000, then fix nvt 300 K (nsinit steps), fix npt iso 1 atm
 * 300->500 K (nsinit), 500 K (5 nsinit), 500->T (nsinit), T (2 nsinit, box lengths averaged, change_box to the averages), fix nvt
 * T (20 nsinit), fix npt T (2 nsinit, averaged, change_box), fix nvt T (nsinit); no SHAKE (commented out in the script).
 * The equilibrated state replaces the registered initial state of the replica (what write_restart init.<mat>_<rep>.bin
 * keeps, :208-210); length[3] = its box lengths (:196-208).  info (may be NULL) [5]: minimiser stop reason (0 energy
 * tolerance, 1 force tolerance, 2 iterations, 3 evaluations, 4 line search), iterations, force evaluations, initial and final
 * potential energy.  LAMMPS' random stream of `velocity create` is not reproduced (own generator, same seed semantics). */
typedef struct {
  int32_t nsteps_equil;    /* nsinit = "molecular dynamics parameters.number of equilibration steps" (init_material.cc:177) */
  double timestep_length;  /* fs */
  double temperature;      /* K, tempt */
  int64_t seed;            /* sseed; 0 = 1234 (init_material_problem.h:167) */
} scema_md_equilparams;
int scema_md_equilibrate(scema_md_engine *e, const char *matid, int32_t replica, const scema_md_equilparams *p, double length[3],
                         double *info);

/* ---- parity / measurement hooks ---- */
/* min_style sd + minimize on a stored state; info[5] as in scema_md_equilibrate */
int scema_md_debug_minimize(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double etol, double ftol,
                            int32_t maxiter, int32_t maxeval, double *info);
/* one run under fix nvt (npt 0) or fix npt ... iso (npt 1) with the target ramped t_start -> t_stop, no SHAKE; lavg (may be
 * NULL) [3]: running average of the box lengths over the two half-run windows */
int scema_md_debug_run_nh(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, int32_t nsteps, double dt,
                          double t_start, double t_stop, int32_t npt, double p_target, double p_period, double *lavg);
/* Static evaluation at the stored state of (qp,mat,rep) (qp_id = SCEMA_MD_QP_NONE: the registered
 * init state): forces [natoms*3], energies[SCEMA_MD_NPART], virials[SCEMA_MD_NPART*6] (kcal/mol). */
int scema_md_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, int32_t use_shake,
                           double *f, double *energies, double *virials, double *info /* [8]: g_ewald,nk,npairs,tdof,... */);
/* Diagnostics of the skin bands of the pair rows: for the replica at position pos of the last run, as the next pair launch
 * would walk its rows: out[0] = K (bands), then K skin entries listed per band, K walked per band, rows with skin entries, rows with a band
 * open, rows with every band open.  cap >= 2 K + 4. */
int scema_md_debug_skin_bands(scema_md_engine *e, int32_t pos, uint64_t *out, int32_t cap);
/* The neighbour rows of a row potential (Stillinger-Weber ... ADP) for the replica at position pos of the last run or
 * static evaluation of such a potential, as its last list build left them: info[6] = atoms n, row capacity, 1 if the rows were built
 * through cells (0: the N^2 build), the cell grid ncell[3] (0 0 0 on the N^2 build).  With cnt and rows non-NULL: cnt[n] entries per row
 * and rows[n][capacity], an entry = atom | image code << 24, ascending by atom; rows_cap (in entries) < n * capacity, or no such run, is
 * an error with a message.  Both builds write the same rows: SCEMA_MD_ROW_CELLS chooses between them (performance only). */
int scema_md_debug_rows(scema_md_engine *e, int32_t pos, int32_t *cnt, int32_t *rows, int64_t rows_cap, int32_t *info);
/* One "run": nsteps of Verlet + SHAKE + NVT (+deform if rates) (+pressure average if press_avg). */
int scema_md_debug_run(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, int32_t nsteps,
                       double dt, double temperature, int32_t nvt, int32_t use_shake, const double *rates,
                       double *press_avg);

/* ---- ReaxFF replicas (md_force_field "reax": lammps_scripts/lammps_scripts_reax) ----
 * configure = what the reax scripts set up in LAMMPS before every run: `pair_style reax/c NULL safezone 50.0 mincap 100000`,
 * `pair_coeff * * <ffield> H C N O` (elements[k] = element of LAMMPS atom type k+1), `fix qeq/reax 1 0.0 10.0 <qeq_tol> reax/c`
 * (in.strain.lammps:10-12, ELASTIC/potential.mod.lammps:5-7); no SHAKE, no k-space, `neigh_modify every 1 delay 0 check no`.
 * qeq_tol <= 0: 1e-6.  skin < 0: default list skin (performance only: the pairs inside the 10 A taper radius do not depend
 * on it).  scema_md_strain_batch configures by itself from MDSim.scripts_folder + "/ffield.reax.2" and H C N O, as the
 * reference's script does, when a simulation asks for force_field "reax" and nothing was configured.  A replica for this
 * path is registered like any other (atom types, masses, box, x, v; no bonds; charges are equilibrated every step). */
int scema_md_reax_configure(scema_md_engine *e, const char *ffield_path, const char *const *elements, int32_t n_elements,
                            double qeq_tol, double skin);
/* which force field the parity hooks (scema_md_debug_run, scema_md_reax_debug_compute) use; strain_batch decides per call
 * from MDSim.force_field */
int scema_md_reax_activate(scema_md_engine *e, int32_t on);
/* parity switches (-1 keeps): exact_gradient 0 = drop the d(SBO)/d(Delta) term of the valence-angle energy for atoms with
 * vlpex >= 0, as USER-REAXC's Valence_Angles is remembered to do (unverifiable here, not energy conserving: DESIGN.md;
 * default 1 = the exact gradient); terms = bit mask of energy-term groups evaluated (31 = all) */
int scema_md_reax_set(scema_md_engine *e, int32_t exact_gradient, int32_t terms, int32_t qeq_maxiter);
/* How a ReaxFF batch is issued on the device -- results do not depend on it.  halves: the number of part batches, each on its own stream (default 2; batches of
   at least four replicas per part), 0 or 1 = one sequence of launches.  overlap: 1 = the bond-order chain of the force stage on a side stream next to the charge
   chain (default), 0 = one after the other.  -1 leaves a setting as it is.  A measurement aid: bench.py times the charge-equilibration sweep
   alone with both off.  (The reference has no counterpart: its LAMMPS ranks run one replica each, stmd_sync.h:583.) */
int scema_md_reax_concurrency(scema_md_engine *e, int32_t halves, int32_t overlap);
/* The same for the OPLS path: on = 1 (default) runs a launch group of 9 simulations and more as two to four part batches on streams of their own, 0 runs it whole
 * (one sequence of launches: what a kernel's time is with the chip to itself), -1 keeps the setting.  Results do not depend on it. */
int scema_md_batch_split(scema_md_engine *e, int32_t on);
/* out[3]: the current settings {batch split, ReaxFF part batches, ReaxFF overlap}, so that a caller that changes them for a measurement can
 * put back exactly what it found */
int scema_md_get_concurrency(const scema_md_engine *e, int32_t *out);
/* PPPM meshes beyond the LDS (more than 18 432 points for the charge assignment, 6 144 for the interpolation; PE-10k's 12 x 12 x 12 is far
 * below both).  mode 1 (default): the tiled kernels -- the mesh cut into bricks in (y, z) that are kept (assignment) or staged with a halo of
 * two rows (interpolation) in LDS; 0: the kernels without LDS of before (global atomics, reads through the caches); -1 keeps the setting.
 * lds_bytes: the LDS budget of the tile rule AND of the whole-mesh tests, 0 = the device default (144 KB), -1 keeps; a test and measurement
 * aid that makes small meshes run as several tiles (16 .. 163 840; a mesh whose smallest brick is beyond it takes the kernels without
 * LDS, scema_md_pppm_paths says so).  Results do not depend on either beyond the order of summation. */
int scema_md_pppm_tiling(scema_md_engine *e, int32_t mode, int32_t lds_bytes);
/* Binned charge assignment (meshes whose padded copy is kept whole in LDS, every nx >= 5, interpolation not tiled): the charged atoms are
 * grouped by nearest grid point once per step (k_pppm_bins) and a lane of the spreading kernel adds the sum of up to a few atoms with one set
 * of 125 LDS atomics.  mode 0: off; 1: on for every launch that is eligible; 2 (default): by the launch policy -- replicas per launch and
 * mean charged atoms per grid point; -1 keeps.  SCEMA_MD_PPPM_BINNED=0/1 in the environment forces 0 / 1 whatever is set here.  Results do
 * not depend on it beyond the order of summation. */
int scema_md_pppm_binning(scema_md_engine *e, int32_t mode);
/* Stream of the bonded kernel.  mode 0: one descriptor per term; 1: the grouped stream of csrc/md_bonded_groups.h -- the dihedrals around
 * one central bond evaluated by one thread (eight positions read once, eight forces added once), every 1-2 / 1-3 special pair inside the
 * bond / angle term that already holds its two atoms; -1: the default (grouped).  SCEMA_MD_BONDED_GROUPED=0/1 in the environment forces
 * 0 / 1 whatever is set here.  The parity hook (scema_md_debug_compute) always runs the per-term stream.  Forces and virials of the two
 * agree to rounding (two formulations of one sum). */
int scema_md_bonded_grouping(scema_md_engine *e, int32_t mode);
/* LDS layout of the staged interpolation kernel (k_pppm_force with the three field grids of a replica in LDS).  mode 0: the dense layout,
 * plane stride nx ny; 1: the plane stride of the rule in csrc/md_pppm_fstride.h, which keeps the stencil points of neighbouring atoms off
 * each other's LDS banks (dense where the padded copy does not fit the LDS budget, would cost a resident workgroup, or the mesh has a
 * dimension of five points or fewer) and 512 instead of 256 threads per workgroup; -1: the default, which is 1.  SCEMA_MD_PPPM_FLAYOUT=0/1 in the environment forces 0 / 1 whatever is
 * set here.  Only where a field point lies in LDS changes; the arithmetic of an atom, and with it every result, is the same in both. */
int scema_md_pppm_force_layout(scema_md_engine *e, int32_t mode);
/* the rule's answer for a mesh and an LDS budget in bytes (0: the device limit): out[3] = {row stride, plane stride (doubles), LDS bytes of
 * the three staged fields}.  A pure host function (no GPU). */
int scema_md_pppm_force_strides(const int32_t grid[3], int32_t lds_bytes, int32_t out[3]);
/* spreading launches of this engine that took the binned kernels so far (a test reads this), or a negative error code */
long long scema_md_pppm_binned_launches(const scema_md_engine *e);
/* out[8], for the last PPPM launch group: {charge assignment: 0 whole mesh in LDS, 1 tiled, 2 global atomics; interpolation: 0 staged, 1 tiled,
 * 2 unstaged; largest tile counts of the assignment in y and z; of the interpolation in y and z (1 1 where the kernel is not the tiled one);
 * the LDS budget in force in bytes; the mode} */
int scema_md_pppm_paths(const scema_md_engine *e, int32_t out[8]);
/* The tile rule as a pure host function (no GPU, no engine): for a mesh grid[3] and an LDS budget (0: the device default) the brick
 * {by, bz} in mesh rows and the tile counts {tiles_y, tiles_z} of which = 0 the charge assignment (nx by bz doubles kept) or 1 the
 * interpolation (3 nx (by + 4)(bz + 4) doubles staged, the halo on tiled axes only); a mesh that fits whole is one tile; z-slabs (by = ny)
 * while one plane / five planes fit; zeros = the smallest brick does not fit (8 nx bytes; 600 nx bytes). */
int scema_md_pppm_tile_shape(const int32_t grid[3], int32_t lds_bytes, int32_t which /* 0 spread, 1 force */, int32_t out[4]);
/* number of batched hipFFT plans the engine holds for PPPM meshes beyond the in-LDS solve (a plan owns a work area and is bound to a stream
 * when it runs: one per mesh size, batch count and stream of a part batch -- a test reads this), or a negative error code */
int scema_md_pppm_plan_count(const scema_md_engine *e);
/* static evaluation: f [natoms*3], eparts[13] (bond, lone pair, over, under, angle, penalty, 3-body conj., torsion, 4-body
 * conj., hydrogen bond, van der Waals, Coulomb, polarisation; kcal/mol), virial[6] (xx,yy,zz,xy,xz,yz), charges q[natoms],
 * info[6]: longest neighbour row, row capacity, bond-row capacity, CG iterations, image search (0 = minimum image), longest bond row */
int scema_md_reax_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *eparts,
                                double *virial, double *q, double *info);
/* out[7]: conjugate-gradient iterations, solves (two systems each), list skin, tolerance, solves finished by the single-workgroup
 * loop, iterations currently issued as batch launches per solve, evaluations repeated with the Jacobi preconditioner of fix qeq/reax
 * because the charge solve did not converge with the engine's own */
int scema_md_reax_stats(const scema_md_engine *e, double *out);

/* ---- Stillinger-Weber replicas (`pair_style sw`: the reference's examples/streched_polyhedron, lammps_scripts_sisw) ----
 * configure = `pair_style sw` + `pair_coeff * * <sw_path> <elements...>` (elements[k] = element of LAMMPS atom type k+1) for the replicas of
 * ONE material id, registered before or after the call; list skin `neighbor <skin> nsq` (skin < 0: 1.0, the example's), rebuilt by the
 * engine's displacement test (`neigh_modify every 1 delay 0 check yes`).  energy_unit 0: the file's epsilon is in eV, as the header of the
 * reference's Si.sw says, and is converted to kcal/mol with 23.060549; 1: epsilon is kcal/mol as written (what LAMMPS 17Nov16 does with
 * that file under the example's `units real`).  Simulations of such a material take the Stillinger-Weber force stage whatever
 * MDSim.force_field says (the example's inputs.json says "opls"): no SHAKE, no k-space, no bonded terms.  An update or run that mixes
 * them with simulations of other materials is refused with SCEMA_MD_ERR_ARG. */
int scema_md_sw_configure(scema_md_engine *e, const char *matid, const char *sw_path, const char *const *elements, int32_t n_elements,
                          int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], two-body and three-body energy (kcal/mol), virial[6] (xx,yy,zz,xy,xz,yz),
 * info[4]: longest neighbour row the build asked for, row capacity, pairs inside their cutoff, triplets evaluated */
int scema_md_sw_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e2, double *e3,
                              double *virial, double *info);
/* The reader of LAMMPS *.sw files as a pure host function (no GPU, no engine).  `#` starts a comment; an entry is three element names and
 * eleven numbers (epsilon sigma a lambda gamma costheta0 A B p q tol) on one line or several; the entries whose three elements are all
 * named are kept.  n_kept: distinct elements named (at most 4, in order of first appearance); type_map[n_elements]: their index per LAMMPS
 * type; values[n_kept][n_kept][n_kept][11] (room for 4*4*4*11): the numbers of entry i j k, epsilon in kcal/mol.  The pair parameters of
 * (i, j) are those of entry i j j, as in pair_sw.cpp.  A missing triplet, a non-numeric field, a short or duplicate entry:
 * SCEMA_MD_ERR_IO with the reason in errbuf. */
int scema_md_sw_read_params(const char *sw_path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                            int32_t *type_map, double *values, char *errbuf, int32_t errcap);

/* ---- Tersoff replicas (`pair_style tersoff`; silicon, carbon, silicon carbide) ----
 * configure = `pair_style tersoff` + `pair_coeff * * <path> <elements...>` (elements[k] = element of LAMMPS atom type k+1) for the replicas
 * of ONE material id, registered before or after the call; list skin as for scema_md_sw_configure (skin < 0: 1.0).  energy_unit 0: A and B
 * of the file are in eV (units metal, as the files LAMMPS ships) and are converted to kcal/mol with 23.060549; 1: kcal/mol as written.
 * Simulations of such a material take the Tersoff force stage whatever MDSim.force_field says: no SHAKE, no k-space, no bonded terms.  An
 * update or run that mixes them with simulations of other materials (Stillinger-Weber ones included) is refused with SCEMA_MD_ERR_ARG.  A
 * material holds ONE attachment: configuring a Tersoff potential for a material that has a Stillinger-Weber one replaces it, and the other
 * way round.  At most 32 neighbours of an atom may lie inside the cutoff R + D; more is an error of the run, never a truncation.
 * A bare replica whose material has nothing attached and whose scripts folder holds no Si.sw configures itself at a scema_md_strain_batch
 * from the line `pair_coeff * * ${locs}/<name>.tersoff <El> ...` of <scripts_folder>/in.strain.lammps (file <scripts_folder>/<name>.tersoff,
 * energy unit eV); a malformed line of that kind is SCEMA_MD_ERR_ARG. */
int scema_md_tersoff_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                               int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], the repulsive energy sum 1/2 fC fR and the bond-order energy sum 1/2 fC b fA (kcal/mol), virial[6]
 * (xx,yy,zz,xy,xz,yz), info[4]: longest neighbour row the build asked for, row capacity, ordered pairs inside their cutoff, ordered (j, k)
 * evaluated for the bond orders */
int scema_md_tersoff_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_rep,
                                   double *e_att, double *virial, double *info);
/* The reader of LAMMPS *.tersoff files as a pure host function (no GPU, no engine).  `#` starts a comment; an entry is three element names
 * and fourteen numbers (m gamma lambda3 c d costheta0 n beta lambda2 B R D lambda1 A) on one line or several; the entries whose three
 * elements are all named are kept.  n_kept, type_map as for scema_md_sw_read_params; values[n_kept][n_kept][n_kept][14] (room for
 * 4*4*4*14): the numbers of entry i j k, A and B in kcal/mol.  n, beta, lambda2, B, lambda1, A and the pair's R, D are those of entry
 * i j j; m, gamma, lambda3, c, d, costheta0 and the R, D of the third atom's cutoff those of entry i j k, as in pair_tersoff.cpp.  A missing
 * triplet, a non-numeric field, a short or duplicate entry, a negative c, d, n, beta, lambda2, B, R, D, lambda1, A or gamma, D > R, m other
 * than 1 or 3, n = 0 in an entry i j j (the switch points of b(zeta) would not exist): SCEMA_MD_ERR_IO with the reason in errbuf. */
int scema_md_tersoff_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                 int32_t *type_map, double *values, char *errbuf, int32_t errcap);

/* ---- the Tersoff forms `pair_style tersoff/mod`, `tersoff/mod/c` (Kumagai et al.: Si.tersoff.mod, Si.tersoff.modc) and `tersoff/zbl`
 * (Devanathan et al.: SiC.tersoff.zbl) ----
 * Each is a kind of its own on the same stage, with everything said of scema_md_tersoff_configure: one attachment per material (configuring
 * replaces a plain Tersoff one and the other way round), the limit of 32 neighbours inside R + D, the refusal of updates and runs that mix
 * kinds (a Tersoff/mod material with a plain Tersoff one included), the energy unit (ZBL: energy_unit 1 also takes the Coulomb constant of
 * `units real`, K / 0.043365121).  One entry point serves tersoff/mod and tersoff/mod/c: a file whose first entry carries 18 numbers is
 * mod/c (the 18th is c0), otherwise c0 = 0.  A bare replica configures itself from `pair_coeff * * ${locs}/<name>.tersoff.mod`, `.tersoff.modc`
 * or `.tersoff.zbl` of in.strain.lammps, searched after *.tersoff and *.eam.alloy.  debug_compute: e_rep is everything without b_ij (the c0
 * term and the ZBL repulsion included), e_att everything that carries it. */
int scema_md_tersoff_mod_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                                   int32_t energy_unit, double skin);
int scema_md_tersoff_mod_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_rep,
                                       double *e_att, double *virial, double *info);
int scema_md_tersoff_zbl_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                                   int32_t energy_unit, double skin);
int scema_md_tersoff_zbl_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_rep,
                                       double *e_att, double *virial, double *info);
/* The readers as pure host functions, as scema_md_tersoff_read_params: values[n_kept][n_kept][n_kept][18] for both forms (room for
 * 4*4*4*18).  mod: beta alpha h eta beta_ters lambda2 B R D lambda1 A n c1 c2 c3 c4 c5 c0, with c0 = 0 for a 17-column file, A, B and c0
 * in kcal/mol; refused: beta_ters other than 1, beta other than 1 or 3, a negative alpha, eta, lambda2, B, R, D, lambda1, A, n, c2, c3, c4
 * or c5, D > R, n = 0 or eta = 0 in an entry i j j, c3 = 0 with -1 <= h <= 1.  zbl: the fourteen numbers of a plain entry, then Z_i Z_j
 * ZBLcut ZBLexpscale; refused: what the plain reader refuses, Z <= 0, a negative ZBLcut or ZBLexpscale. */
int scema_md_tersoff_mod_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                     int32_t *type_map, double *values, char *errbuf, int32_t errcap);
int scema_md_tersoff_zbl_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                     int32_t *type_map, double *values, char *errbuf, int32_t errcap);

/* ---- embedded-atom replicas (`pair_style eam/alloy`; metals and their alloys) ----
 * configure = `pair_style eam/alloy` + `pair_coeff * * <path> <elements...>` (elements[k] = element of LAMMPS atom type k+1, in any order,
 * repeats allowed, at most 4 distinct) for the replicas of ONE material id, registered before or after the call; <path> is a DYNAMO setfl
 * file; list skin as for scema_md_sw_configure (skin < 0: 1.0).  energy_unit 0: F and r phi of the file are in eV and eV A (units metal)
 * and are converted to kcal/mol with 23.060549; 1: as written.  The density has no unit.  The file's masses are read and checked, not
 * applied: masses come from the replica.  The tables become cubic splines on the file's own knots (seven coefficients per knot, the
 * derivative exactly that of the cubic: forces are the exact gradient of the energy); above rhomax = (Nrho - 1) drho the embedding energy
 * continues linearly.  Simulations of such a material take the embedded-atom force stage whatever MDSim.force_field says: no SHAKE, no
 * k-space, no bonded terms; an atom may have any number of neighbours inside the cutoff.  An update or run that mixes them with
 * simulations of other materials is refused with SCEMA_MD_ERR_ARG.  A material holds ONE attachment: configuring replaces whatever it
 * held, of any kind.  A bare replica whose material has nothing attached, whose scripts folder holds no Si.sw and whose in.strain.lammps
 * names no *.tersoff file configures itself at a scema_md_strain_batch from the line `pair_coeff * * ${locs}/<name>.eam.alloy <El> ...`
 * of <scripts_folder>/in.strain.lammps (energy unit eV); a malformed line of that kind is SCEMA_MD_ERR_ARG.  Not built: eam/fs, funcfl
 * `pair_style eam`, tables of different spacing. */
int scema_md_eam_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                           int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], the pair energy 1/2 sum phi and the embedding energy sum F(rho) (kcal/mol), virial[6]
 * (xx,yy,zz,xy,xz,yz), info[4]: longest neighbour row the build asked for, row capacity, ordered pairs inside the cutoff, atoms whose
 * density lies above rhomax */
int scema_md_eam_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_pair,
                               double *e_embed, double *virial, double *info);
/* The reader of setfl files as a pure host function (no GPU, no engine): three comment lines; `Nelements name ...`; `Nrho drho Nr dr
 * cutoff`; per element `Z mass a0 lattice`, Nrho values of F, Nr values of rho(r); then for every pair i >= j in file order Nr values of
 * r phi_ij(r); numbers free-format across lines.  n_kept, type_map as for scema_md_sw_read_params; head[8]: Nrho, drho, Nr, dr, cutoff,
 * rhomax, the number of doubles of the tables, 0; masses[n_kept] (room for 4); tables (may be NULL; tables_cap doubles of room): per kept
 * element the records of F ([Nrho][4] value {s3 s4 s5 s6}, then [Nrho][4] derivative {s0 s1 s2 0}) and of rho ([Nr][4] twice), then per
 * kept pair i >= j those of r phi, F and r phi in kcal/mol.  A short or truncated file, a non-numeric field, Nr or Nrho below 5, dr, drho
 * or the cutoff not positive, a cutoff beyond (Nr - 1) dr, an element that is not in the file, counts that the file's length cannot hold:
 * SCEMA_MD_ERR_IO with the reason in errbuf. */
int scema_md_eam_read_setfl(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                            int32_t *type_map, double *head, double *masses, double *tables, int64_t tables_cap, char *errbuf, int32_t errcap);

/* ---- Vashishta replicas (`pair_style vashishta`; SiC, SiO2, Al2O3, InP) ----
 * configure = `pair_style vashishta` + `pair_coeff * * <path> <elements...>` (elements[k] = element of LAMMPS atom type k+1, at most 4
 * distinct) for the replicas of ONE material id, registered before or after the call; list skin as for scema_md_sw_configure (skin < 0:
 * 1.0).  energy_unit 0: H, D, W and B of the file are eV-based (units metal), the Coulomb constant K is 14.399645 eV A, and everything is
 * converted to kcal/mol with 23.060549; 1: the numbers as written and K = 332.06371 (units real).  The form:
 *   U(r) = H r^-eta + K Zi Zj exp(-r/lambda1)/r - D exp(-r/lambda4)/r^4 - W/r^6,  E2(r) = U(r) - U(rc) - (r - rc) U'(rc) for r < rc;
 *   E3 = B dc^2/(1 + C dc^2) exp(gamma_ij/(r_ij - r0_ij) + gamma_ik/(r_ik - r0_ik)), dc = cos theta - costheta0, for r_ij < r0_ij, r_ik < r0_ik.
 * Simulations of such a material take the Vashishta force stage whatever MDSim.force_field says: no SHAKE, no k-space, no bonded terms.
 * The pair term takes any number of neighbours inside rc; at most 32 neighbours of an atom may lie inside r0, the three-body range: more
 * is an error of the run, never a truncation.  An update or run that mixes them with simulations of other materials is refused with
 * SCEMA_MD_ERR_ARG.  A material holds ONE attachment: configuring replaces whatever it held, of any kind.  A bare replica whose material
 * has nothing attached configures itself at a scema_md_strain_batch from the line `pair_coeff * * ${locs}/<name>.vashishta <El> ...` of
 * <scripts_folder>/in.strain.lammps (energy unit eV), searched after every other extension; a malformed line of that kind is
 * SCEMA_MD_ERR_ARG.  Not built: vashishta/table. */
int scema_md_vashishta_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                                 int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], two-body and three-body energy (kcal/mol), virial[6] (xx,yy,zz,xy,xz,yz), info[4]: longest neighbour row
 * the build asked for, row capacity, ordered pairs inside rc (each pair counts at both ends), pairs (a, b) of the lists inside r0 */
int scema_md_vashishta_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e2, double *e3,
                                     double *virial, double *info);
/* The reader of LAMMPS *.vashishta files as a pure host function (no GPU, no engine).  `#` starts a comment; an entry is three element
 * names and fourteen numbers (H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta0) on one line or several; the entries whose three
 * elements are all named are kept.  n_kept, type_map as for scema_md_sw_read_params; values[n_kept][n_kept][n_kept][14] (room for
 * 4*4*4*14): the numbers of entry i j k, H, D, W and B in kcal/mol.  H eta Zi Zj lambda1 D lambda4 W rc and the arm's gamma, r0 of a pair
 * (i, j) are those of entry i j j; B, C, costheta0 of a triplet those of entry i j k, as in pair_vashishta.cpp.  A lambda of 0 means
 * exp(...) = 1.  A missing triplet, a non-numeric field, a short or duplicate entry; in an entry i j j: rc <= 0, eta <= 0 with H != 0, a
 * negative lambda1, lambda4, gamma or r0, r0 > rc; a negative C in any entry; entries i j j and j i i whose rc or r0 differ (a pair has
 * one cutoff at both ends): SCEMA_MD_ERR_IO with the reason in errbuf. */
int scema_md_vashishta_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                   int32_t *type_map, double *values, char *errbuf, int32_t errcap);

/* ---- Angular-dependent potential (`pair_style adp`; Mishin, Mehl and Papaconstantopoulos, Acta Mater. 53, 4029 (2005): Cu-Ta, Al-Cu,
 * U-Mo, Fe-Ni, bcc metals) ----
 * configure = `pair_style adp` + `pair_coeff * * <path> <elements...>` (elements[k] = element of LAMMPS atom type k+1, at most 4 distinct)
 * for the replicas of ONE material id; list skin and energy_unit as for scema_md_eam_configure, u and w being converted with the square
 * root of 23.060549 at energy_unit 0.  The form, with d = x_j - x_i over 0 < r^2 < cutoff^2:
 *   rho_i = sum_j rho_{el(j)}(r),  mu_i[a] = sum_j u_{el(i)el(j)}(r) d[a],  lam_i[ab] = sum_j w_{el(i)el(j)}(r) d[a] d[b],  nu_i = tr lam_i
 *   E = sum_i [F(rho_i) + 1/2 |mu_i|^2 + 1/2 sum_ab lam_i[ab]^2 - nu_i^2 / 6] + 1/2 sum_i sum_j phi(r)
 * with F continued linearly above rhomax as for eam/alloy.  Any number of neighbours is taken.  Simulations of such a material take the
 * ADP force stage whatever MDSim.force_field says.  An update or run that mixes them with simulations of other materials is refused with
 * SCEMA_MD_ERR_ARG.  A material holds ONE attachment: configuring replaces whatever it held, of any kind.  A bare replica whose material
 * has nothing attached configures itself at a scema_md_strain_batch from the line `pair_coeff * * ${locs}/<name>.adp <El> ...` of
 * <scripts_folder>/in.strain.lammps (energy unit eV), searched after every other extension. */
int scema_md_adp_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                           int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], pair energy (1/2 sum phi) and many-body energy (embedding plus the angular terms; kcal/mol), virial[6]
 * (xx,yy,zz,xy,xz,yz), info[4]: longest neighbour row the build asked for, row capacity, ordered pairs inside the cutoff, atoms whose
 * density lies above rhomax */
int scema_md_adp_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_pair, double *e_manybody,
                               double *virial, double *info);
/* The reader of extended setfl files (*.adp) as a pure host function: the arguments of scema_md_eam_read_setfl.  The file is a setfl file
 * through its r phi tables; then follow, for every pair i >= j in file order, Nr values of u_ij(r), then in the same order Nr values of
 * w_ij(r), as written (not multiplied by r).  In `tables` the records of u (kept pairs i >= j), then those of w, follow the r phi
 * records; head[6] counts them.  The refusals of scema_md_eam_read_setfl, and a file that ends inside the u or the w tables. */
int scema_md_adp_read_setfl(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                            int32_t *type_map, double *head, double *masses, double *tables, int64_t tables_cap, char *errbuf, int32_t errcap);

/* ---- EDIP replicas (`pair_style edip`: silicon, Justo, Bazant, Kaxiras, Bulatov and Yip, Phys. Rev. B 58, 2539 (1998), Si.edip;
 * `pair_style edip/multi`: SiC) ----
 * configure = `pair_style edip` (or `edip/multi`) + `pair_coeff * * <path> <elements...>` (elements[k] = element of LAMMPS atom type k+1,
 * at most 4 distinct) for the replicas of ONE material id, registered before or after the call; list skin as for scema_md_sw_configure
 * (skin < 0: 1.0).  energy_unit 0: A and lambda of the file are eV (units metal) and are converted to kcal/mol with 23.060549; 1: as
 * written.  The form, evaluated in closed form in FP64 (LAMMPS interpolates grids; parity with it is unpinned):
 *   f(r) = 1 (r <= c), exp(alpha/(1 - x^-3)) with x = (r - c)/(a - c) (c < r < a), 0 (r >= a);  Z_i = sum_m f(r_im);
 *   V2(r,Z) = A [(B/r)^rho - exp(-beta Z^2)] exp(sigma/(r - a));  g(r) = exp(gamma/(r - a));  Q(Z) = Q0 exp(-mu Z);
 *   tau(Z) = u1 + u2 (u3 exp(-u4 Z) - exp(-2 u4 Z));  h(l,Z) = lambda [(1 - exp(-Q (l + tau)^2)) + eta Q (l + tau)^2];
 *   E = sum_i [ sum_{j != i} V2(r_ij, Z_i) + sum_{j<k} g(r_ij) g(r_ik) h(cos theta_jik, Z_i) ],  the pair sum over ordered pairs (no 1/2).
 * Forces are the exact gradient, the part (dE_i/dZ_i) f'(r_im) on every neighbour m of i included.  Simulations of such a material take
 * the EDIP force stage whatever MDSim.force_field says: no SHAKE, no k-space, no bonded terms.  At most 32 neighbours of an atom may lie
 * inside a (cutoffA): more is an error of the run, never a truncation.  An update or run that mixes them with simulations of other
 * materials is refused with SCEMA_MD_ERR_ARG.  A material holds ONE attachment: configuring replaces whatever it held, of any kind.  A
 * bare replica whose material has nothing attached configures itself at a scema_md_strain_batch from the line
 * `pair_coeff * * ${locs}/<name>.edip <El> ...` of <scripts_folder>/in.strain.lammps (energy unit eV), searched after every other
 * extension; a malformed line of that kind is SCEMA_MD_ERR_ARG.  Not built: LAMMPS' interpolation grids. */
int scema_md_edip_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                            int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], two-body and three-body energy (kcal/mol), virial[6] (xx,yy,zz,xy,xz,yz), info[4]: longest neighbour row
 * the build asked for, row capacity, ordered pairs inside a (each pair counts at both ends), triplets */
int scema_md_edip_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e2, double *e3,
                                double *virial, double *info);
/* The reader of LAMMPS *.edip files as a pure host function (no GPU, no engine).  `#` starts a comment; an entry is three element names and
 * seventeen numbers (A B cutoffA cutoffC alpha beta eta gamma lambda mu rho sigma Q0 u1 u2 u3 u4) on one line or several; the entries
 * whose three elements are all named are kept.  n_kept, type_map as for scema_md_sw_read_params; values[n_kept][n_kept][n_kept][17] (room
 * for 4*4*4*17): the numbers of entry i j k, A and lambda in kcal/mol.  A B rho beta sigma a c alpha gamma of a pair (i, j) are those of
 * entry i j j; lambda eta Q0 mu u1..u4 of a triplet those of entry i j k; the arm g of a triplet takes gamma and a of its own pair.  A
 * missing triplet, a non-numeric field, a short or duplicate entry; in an entry i j j: cutoffA <= 0, cutoffC < 0, cutoffC >= cutoffA, a
 * negative alpha, sigma, gamma or rho, B <= 0 with A != 0; entries i j k and i k j whose eight triplet numbers differ (the sum over
 * j < k must not depend on the row's order); entries i j j and j i i whose cutoffA differ (a pair has one cutoff at both ends):
 * SCEMA_MD_ERR_IO with the reason in errbuf. */
int scema_md_edip_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                              int32_t *type_map, double *values, char *errbuf, int32_t errcap);

/* ---- spline-MEAM replicas (`pair_style meam/spline`: Lenosky et al., Modelling Simul. Mater. Sci. Eng. 8, 825 (2000); Hennig et al.,
 * Phys. Rev. B 78, 054121 (2008): Ti, Zr, Nb, Mo, Si, Ti-O) ----
 * configure = `pair_style meam/spline` + `pair_coeff * * <path> <elements...>` (elements[k] = element of LAMMPS atom type k+1, at most 2
 * distinct; the old one-element format names no element and takes any) for the replicas of ONE material id, registered before or after
 * the call; list skin as for scema_md_sw_configure (skin < 0: 1.0).  energy_unit 0: phi and U of the file are eV (units metal) and are
 * converted to kcal/mol with 23.060549; 1: as written.  The form:
 *   E = sum_{i<j} phi_{ti tj}(r_ij) + sum_i [U_ti(rho_i) - U_ti(0)],
 *   rho_i = sum_j rho_tj(r_ij) + sum_{j<k} f_tj(r_ij) f_tk(r_ik) g_{tj tk}(cos theta_jik),
 * every function a clamped cubic spline through its knots (at most 32, equidistant or not) with the end slopes of the file and second
 * derivatives from the tridiagonal solve (the file's third column is read and ignored), continued linearly beyond either end.  phi, rho
 * and f are zero at and beyond their last knot, and a file in which one of them does not end with value 0 and slope 0 is refused; LAMMPS,
 * as remembered, tests one global cutoff and lets rho and f continue linearly up to it -- the same thing for such a file (unpinned:
 * DESIGN.md 7o).  Forces are the exact gradient.  Simulations of such a material take the spline-MEAM force stage whatever
 * MDSim.force_field says: no SHAKE, no k-space, no bonded terms.  At most 32 neighbours of an atom may lie inside the last knot of f, the
 * three-body range: more is an error of the run, never a truncation; inside the largest last knot (cutmax) any number is taken.  An update
 * or run that mixes them with simulations of other materials is refused with SCEMA_MD_ERR_ARG.  A material holds ONE attachment:
 * configuring replaces whatever it held, of any kind.  A bare replica whose material has nothing attached configures itself at a
 * scema_md_strain_batch from the line `pair_coeff * * ${locs}/<name>.meam.spline <El> ...` of <scripts_folder>/in.strain.lammps (energy
 * unit eV), searched after every other extension; a malformed line of that kind is SCEMA_MD_ERR_ARG.  Not built: `meam/sw/spline`. */
int scema_md_meam_spline_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                                   int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], pair energy sum phi and embedding energy sum U(rho) - U(0) (kcal/mol), virial[6] (xx,yy,zz,xy,xz,yz),
 * info[4]: longest neighbour row the build asked for, row capacity, ordered pairs inside cutmax (each pair counts at both ends), triplets
 * (pairs of the lists inside f's last knot) */
int scema_md_meam_spline_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_pair,
                                       double *e_embed, double *virial, double *info);
/* The reader of meam/spline files as a pure host function (no GPU, no engine), both formats: old (a comment line, then phi rho U f g, each
 * `N`, `d0 dN`, one skipped line, N lines `x y y2`) and new (a comment line, `meam/spline <n> <El1> .. <Eln>`, then the families phi rho U f
 * g, pair families as the upper triangle row-major, each spline `spline3eq`, `N`, `d0 dN`, N lines `x y y2`).  n_kept, type_map as for
 * scema_md_sw_read_params; the splines of the elements kept stand in the file's order (phi: n (n + 1) / 2, rho, U, f: n each, g), 12 at
 * most: knots[12] their knot counts (0 beyond the last), head[8] = cutmax, number of splines, U(0) [2], cut_f [2][2] (the last knot of f of
 * the second index' element), values[12][4 + 3 * 32] = d0, dN, 1 where the knots are equidistant, the inverse spacing there, x[32], y[32],
 * y2[32], phi and U in kcal/mol.  Refused with SCEMA_MD_ERR_IO and the reason, which names the line, in errbuf: a truncated file, N < 2 or
 * N > 32, knots not strictly ascending, a word that is no finite number, a missing `spline3eq`, an element count that disagrees with the
 * header's list, more than 2 elements kept, an empty or NULL name, a name the file lacks, a phi, rho or f that does not end with value
 * 0 and slope 0. */
int scema_md_meam_spline_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                     int32_t *type_map, int32_t *knots, double *head, double *values, char *errbuf, int32_t errcap);
/* spline `fn` of that list at the points x[n]: y and dy/dx, by the code the kernels run (meam_spline/ms_core.h ms_eval); mode 0: the
 * interval from the inverse spacing where the knots are equidistant, by bisection elsewhere; mode 1: by bisection always (the two agree
 * bit for bit).  fn or mode out of range: SCEMA_MD_ERR_ARG */
int scema_md_meam_spline_eval(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t fn, int32_t mode,
                              const double *x, int32_t n, double *y, double *dy, char *errbuf, int32_t errcap);

/* ---- ionic replicas (`pair_style born/coul/dsf`; rock-salt halides, MgO, UO2, Buckingham and Born-Mayer-Huggins oxides and glasses) ----
 * The first row stage that reads charges: the ones registered with the replica (scema_md_system.charge).  LAMMPS has no parameter file
 * for this style: `path` is any text file that holds the script lines themselves (in.strain.lammps included); blank-separated words,
 * `#` starts a comment, every other command is ignored:
 *   pair_style born/coul/dsf <alpha> <cut_lj> [<cut_coul>]     (cut_coul defaults to cut_lj)
 *   pair_coeff I J A rho sigma C D [cut_lj]                    (I <= J: numeric types from 1, or `*` alone for either)
 *   units real|metal                                           (optional; must not contradict energy_unit)
 * for the replicas of ONE material id, registered before or after the call; list skin as for scema_md_sw_configure (skin < 0: 1.0).
 * energy_unit 0: A, C and D are eV-based (units metal), K = 14.399645 eV A, everything converted to kcal/mol with 23.060549; 1: the
 * numbers as written and K = 332.06371 (units real).  The form, for a pair of types ti, tj, charges q_i, q_j at distance r:
 *   E_born = A exp((sigma - r)/rho) - C/r^6 + D/r^8                              r < cut_lj[ti][tj], not shifted (no pair_modify shift)
 *   E_coul = K q_i q_j [erfc(alpha r)/r - erfc(alpha rc)/rc + f_s (r - rc)]      r < rc = cut_coul
 *   f_s    = erfc(alpha rc)/rc^2 + (2 alpha/sqrt(pi)) exp(-alpha^2 rc^2)/rc
 *   E_self = -K q_i^2 [e_s/2 + alpha/sqrt(pi)] per atom, e_s = erfc(alpha rc)/rc + f_s rc
 * with forces the exact gradients (the Coulomb force is K q_i q_j [erfc(alpha r)/r^2 + (2 alpha/sqrt(pi)) exp(-alpha^2 r^2)/r - f_s]);
 * the self term has no force and no virial.  The fragment's types are 1 .. the largest type a pair_coeff line names (4 at most; where
 * every line says `*`, all 4); an atom of a type beyond them is SCEMA_MD_ERR_ARG at the run.  Any number of neighbours is taken.
 * Simulations of such a material take this force stage whatever MDSim.force_field says: no SHAKE, no k-space, no bonded terms.  An
 * update or run that mixes them with simulations of other materials is refused with SCEMA_MD_ERR_ARG.  A material holds ONE attachment:
 * configuring replaces whatever it held, of any kind.  A replica without topology, with zero Lennard-Jones coefficients, that holds
 * charges and whose material has nothing attached configures itself at a scema_md_strain_batch if <scripts_folder>/in.strain.lammps
 * holds a `pair_style born/coul/dsf` line, from that script's own lines (energy unit 1 iff it says `units real`); lines the reader
 * refuses are SCEMA_MD_ERR_ARG; without such a line nothing changes for the replica.  The long-range form, born/coul/long and
 * buck/coul/long with an Ewald sum, is scema_md_born_long_configure below.  Not built: born/coul/wolf, pair_modify shift. */
int scema_md_born_dsf_configure(scema_md_engine *e, const char *matid, const char *path, int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], e_born, e_coul with the self term (kcal/mol), virial[6] (xx,yy,zz,xy,xz,yz), info[4]: longest
 * neighbour row the build asked for, row capacity, ordered pairs inside cutmax (the largest of all cutoffs; each pair counts at both
 * ends), ordered pairs inside cut_coul */
int scema_md_born_dsf_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_born, double *e_coul,
                                    double *virial, double *info);
/* The reader as a pure host function (no GPU, no engine).  n_types: the fragment's types; head[6]: alpha, cut_coul, e_s, f_s, K
 * (kcal A/mol), cutmax; values[n_types][n_types][6] (room for 4*4*6): A rho sigma C D cut_lj of every ordered pair, A, C and D in
 * kcal/mol.  Refused with SCEMA_MD_ERR_IO and "<path> line <n>: <reason>" in errbuf: no pair_style line (line 0) or two of them; another
 * pair style; alpha <= 0, a cutoff <= 0, rho <= 0; a word that is not a finite number, a missing or surplus word; I > J, a range m*n, a
 * type below 1 or above 4; a pair I <= J of the fragment's types that is never set (there is no mixing rule); a units line that is
 * neither real nor metal or that contradicts energy_unit. */
int scema_md_born_dsf_read_params(const char *path, int32_t energy_unit, int32_t *n_types, double *head, double *values, char *errbuf, int32_t errcap);
/* bd_pair of the kernel (ionic/bd_core.h) on the host: out[n][4] = e_born, e_coul, and the force factors fb, fc (force on i =
 * -(fb + fc)(x_j - x_i)) of a pair of types ti, tj (from 0) and charges qi, qj at the distances r[n]; e_self[2]: the self energies */
int scema_md_born_dsf_eval(const char *path, int32_t energy_unit, int32_t ti, int32_t tj, double qi, double qj, const double *r, int32_t n, double *out,
                           double *e_self, char *errbuf, int32_t errcap);

/* ---- ionic replicas with an Ewald sum or a PPPM mesh (`pair_style born/coul/long`, `pair_style buck/coul/long`, `kspace_style
 * ewald|pppm <accuracy>`) ----
 * The form ionic models are fitted with: the Born-Mayer-Huggins term of born/coul/dsf and the Coulomb sum split by Ewald's method, the
 * reciprocal part summed plainly over a k list where the list fits (512 ions of rock salt at 1e-5 need 709 k-vectors) and on a PPPM
 * mesh beyond it (scema_md_born_long_kspace below).  `path` is any
 * text file that holds the script lines themselves (in.strain.lammps included):
 *   pair_style born/coul/long <cut_lj> [<cut_coul>]   with   pair_coeff I J A rho sigma C D [cut_lj]
 *   pair_style buck/coul/long <cut_lj> [<cut_coul>]   with   pair_coeff I J A rho C [cut_lj]          (sigma = 0, D = 0 of the same table)
 *   kspace_style ewald|pppm <accuracy>                (required; `pppm` is honoured as the Ewald sum at that accuracy, the sum PPPM
 *                                                      approximates, where the k list fits, and runs on the mesh beyond it; a
 *                                                      kspace_modify line is refused: none of its options is honoured)
 *   units real|metal                                  (optional; must not contradict energy_unit)
 * Types, `*`, energy_unit, K, skin and the rules of attachment are those of scema_md_born_dsf_configure.  The form:
 *   E_born  = A exp((sigma - r)/rho) - C/r^6 + D/r^8                         r < cut_lj[ti][tj], not shifted
 *   E_real  = K q_i q_j erfc(g r)/r                                          r < cut_coul, not shifted
 *   E_recip = (2 pi K/V) sum_{k != 0} exp(-k^2/4g^2)/k^2 |S(k)|^2            S(k) = sum_i q_i exp(i k.r_i)
 *   E_self  = -K g/sqrt(pi) sum q_i^2 - K pi (sum q_i)^2/(2 g^2 V)           (the second term: the neutralising background)
 * with forces the exact gradients and the virial the strain derivative of the whole energy at fixed g and fixed integer k triples (the
 * background term included, which LAMMPS leaves out of its virial).  g_ewald and the triples are set up per run from the run's start box,
 * the material's cut_coul and accuracy and the replica's charges, by the rule of `kspace_style ewald` (g from the accuracy, a kmax search
 * per dimension, the Cartesian sphere); the triples stay over the run while fix deform moves the box, and a box flip re-expresses them.
 * A replica whose list exceeds 4096 k-vectors, or an index of 20, is refused with SCEMA_MD_ERR_ARG under `kspace_style ewald` and runs
 * on the mesh under `kspace_style pppm` (scema_md_born_long_kspace).  Forces repeat bit for bit on either solver.  A charged topology-free replica with nothing attached configures itself from a
 * `pair_style born/coul/long` or `buck/coul/long` line of <scripts_folder>/in.strain.lammps, after the born/coul/dsf search. */
int scema_md_born_long_configure(scema_md_engine *e, const char *matid, const char *path, int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], e_born, e_coul (real space, reciprocal space, self and background; kcal/mol), virial[6]
 * (xx,yy,zz,xy,xz,yz), info[6]: the four numbers of scema_md_born_dsf_debug_compute, then the k-vectors of the half space and g_ewald */
int scema_md_born_long_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_born, double *e_coul,
                                     double *virial, double *info);
/* Which reciprocal solver the replicas of a Born/long material get, decided per replica and run.  mode 0 (the default): the Ewald sum
 * wherever its k list fits, whatever the script's solver word; beyond the limits a `kspace_style ewald` script is refused and a
 * `kspace_style pppm` script runs on the mesh.  mode 1: the mesh for every replica.  mode 2: the Ewald sum, refused beyond its limits.
 * The mesh is PPPM as LAMMPS' `kspace_style pppm` does it: order-5 assignment, ik differentiation, the optimal influence function of the
 * step's box, grid and g_ewald per run from the run's start box (set_grid_global, adjust_gewald), fixed over the run; the charge grid is
 * summed in 64-bit fixed point, so forces repeat bit for bit.  On the mesh info[4] of the static evaluation (the k-vectors) is 0 and
 * info[5] the adjusted g_ewald.  Refused with SCEMA_MD_ERR_ARG when a run starts: a mesh of more than 4 194 304 points, a mesh dimension
 * that reaches the search cap of 4096.  SCEMA_MD_ERR_ARG here: an unknown material, one without a Born/long potential, an unknown mode. */
int scema_md_born_long_kspace(scema_md_engine *e, const char *matid, int32_t mode);
/* grid[3]: the mesh of the last scema_md_born_long_debug_compute, zeros if it ran the Ewald sum */
int scema_md_born_long_last_mesh(scema_md_engine *e, int32_t *grid);
/* The reader as a pure host function (no GPU, no engine).  n_types: the fragment's types; head[6]: cut_coul, accuracy, solver (0 ewald,
 * 1 pppm), K (kcal A/mol), cutmax, style (0 born/coul/long, 1 buck/coul/long); values[n_types][n_types][6] (room for 4*4*6): A rho sigma
 * C D cut_lj of every ordered pair, A, C and D in kcal/mol.  Refused with SCEMA_MD_ERR_IO and "<path> line <n>: <reason>" in errbuf: what
 * scema_md_born_dsf_read_params refuses (alpha apart), and no kspace_style line (line 0) or two of them, a solver that is neither ewald
 * nor pppm, an accuracy <= 0 or >= 1, a kspace_modify line, a pair_coeff line with the word count of the other style. */
int scema_md_born_long_read_params(const char *path, int32_t energy_unit, int32_t *n_types, double *head, double *values, char *errbuf, int32_t errcap);
/* bl_pair of the kernel (ionic/bl_core.h) on the host at a given g_ewald: out[n][4] = e_born, e_real, and the force factors fb, fc (force
 * on i = -(fb + fc)(x_j - x_i)) of a pair of types ti, tj (from 0) and charges qi, qj at the distances r[n] */
int scema_md_born_long_eval(const char *path, int32_t energy_unit, double g_ewald, int32_t ti, int32_t tj, double qi, double qj, const double *r,
                            int32_t n, double *out, char *errbuf, int32_t errcap);
/* The k-space set-up a run would use for this box (xlo ylo zlo xhi yhi zhi xy xz yz), as a pure host function: g_ewald, kmax[3] (the
 * largest |n_d| of the list), nk and the integer triples [nk][3] (triples may be null; triples_cap counts triples) for a replica of
 * natoms atoms with sum q^2 = qsqsum under the cut_coul and accuracy of `path` */
int scema_md_born_long_kvectors(const char *path, int32_t energy_unit, const double *box, int32_t natoms, double qsqsum, double *g_ewald, int32_t *kmax,
                                int32_t *nk, int32_t *triples, int32_t triples_cap, char *errbuf, int32_t errcap);
/* The mesh counterpart: the adjusted g_ewald and the mesh grid[3] a run on the mesh solver would use for this box.  A mesh the solver
 * refuses is SCEMA_MD_ERR_ARG with the refusal in errbuf; g_ewald and grid are filled in all the same. */
int scema_md_born_long_mesh(const char *path, int32_t energy_unit, const double *box, int32_t natoms, double qsqsum, double *g_ewald, int32_t *grid,
                            char *errbuf, int32_t errcap);

/* ---- embedded-atom replicas with a long-range Coulomb sum (`pair_style hybrid/overlay coul/long <cut_coul> eam/alloy`, `kspace_style
 * ewald|pppm <accuracy>`) ----
 * The many-body form oxide models of the Cooper-Rushton-Grimes kind are written in (UO2, ThO2, CeO2 and their mixed oxides): the
 * embedded-atom terms of scema_md_eam_configure on a setfl file plus the Coulomb sum of scema_md_born_long_configure over the replica's
 * charges, the first stage made of two potentials.  `script_path` is any text file that holds the script lines themselves
 * (in.strain.lammps included); blank-separated words, `#` starts a comment, every other command is ignored:
 *   units metal|real                                          (optional; must not contradict energy_unit)
 *   pair_style hybrid/overlay coul/long <cut_coul> eam/alloy  (the two sub-styles in either order)
 *   pair_coeff * * coul/long
 *   pair_coeff * * eam/alloy <file> <El> ...                  (one element per atom type)
 *   kspace_style ewald|pppm <accuracy>
 * <file> with a `${locs}/` prefix, or a relative name, is taken relative to the script's own folder; an absolute path as given.
 * energy_unit 0: the setfl tables are eV and are converted with 23.060549, K = 14.399645 eV A; 1: as written, K = 332.06371.  The form:
 *   E_eam  = sum_i F(rho_i) + 1/2 sum phi(r)                                over 0 < r^2 < (setfl cutoff)^2, as scema_md_eam_configure
 *   E_coul = the four Coulomb terms of scema_md_born_long_configure        real space inside cut_coul, which may lie on either side of
 *                                                                          the setfl cutoff
 * One fused real-space kernel walks an atom's row once for both; the reciprocal part (Ewald sum or PPPM mesh per replica and run,
 * scema_md_eam_coul_kspace), its limits and refusals, the box flips and the rules of attachment and skin are those of the Born/long
 * stage.  Forces repeat bit for bit.  Refused with SCEMA_MD_ERR_IO and "<path> line <n>: <reason>": a pair style that is not
 * hybrid/overlay, a third or another sub-style, either pair_coeff line missing or given twice, NULL as an element, no kspace_style line
 * or two of them, a kspace_modify line, cut_coul <= 0, an accuracy outside (0, 1), and everything scema_md_eam_read_setfl refuses (its
 * message is passed on).  A charged topology-free replica with nothing attached configures itself from such a `pair_style
 * hybrid/overlay` line of <scripts_folder>/in.strain.lammps, searched after the two ionic styles; script lines the reader refuses there
 * are SCEMA_MD_ERR_ARG, as for the two ionic styles (the request cannot run), while the setfl file's refusals stay SCEMA_MD_ERR_IO.
 * Left on that row: eam/fs and funcfl
 * readers, other sub-style pairs under hybrid/overlay, charge equilibration, more than four elements. */
int scema_md_eam_coul_configure(scema_md_engine *e, const char *matid, const char *script_path, int32_t energy_unit, double skin);
/* static evaluation: f [natoms*3], e_eam (embedding and pair energy), e_coul (real space, reciprocal space, self and background;
 * kcal/mol), virial[6] (xx,yy,zz,xy,xz,yz), info[6]: that of scema_md_born_long_debug_compute with info[2] = ordered pairs inside the
 * setfl cutoff (info[3]: inside cut_coul) */
int scema_md_eam_coul_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_eam, double *e_coul,
                                    double *virial, double *info);
/* the three modes of scema_md_born_long_kspace for a material of this kind */
int scema_md_eam_coul_kspace(scema_md_engine *e, const char *matid, int32_t mode);
/* grid[3]: the mesh of the last scema_md_eam_coul_debug_compute, zeros if it ran the Ewald sum */
int scema_md_eam_coul_last_mesh(scema_md_engine *e, int32_t *grid);
/* The reader as a pure host function (no GPU, no engine; energy_unit may be -1: 1 iff the script says `units real`).  head[6]: cut_coul,
 * accuracy, solver (0 ewald, 1 pppm), K (kcal A/mol), cutmax = max(setfl cutoff, cut_coul), the setfl cutoff; n_types and
 * type_map[n_types] (room for type_cap): the element of the tables per atom type; setfl_path (room for setfl_cap bytes): the resolved
 * file.  Any output may be null.  Refusals as for scema_md_eam_coul_configure, in errbuf. */
int scema_md_eam_coul_read_params(const char *path, int32_t energy_unit, double *head, int32_t *n_types, int32_t *type_map, int32_t type_cap,
                                  char *setfl_path, int32_t setfl_cap, char *errbuf, int32_t errcap);

typedef struct {
  int64_t pair_launches;     /* timed pair-kernel launches */
  double pair_ms;             /* sum of their HIP-event durations */
  double pair_alg_bytes;      /* algorithmic bytes of those launches, SURVEY.md 8(d) formula */
  int64_t md_steps;           /* simulation-steps advanced (sum over simulations) */
  int64_t neigh_builds;
  double unique_pairs_per_sim;/* average unique pairs within cutoff+skin at the last build */
  int64_t evals;
  double list_skin_mean;      /* mean neighbour-list skin of those evaluations: params.skin + the adaptive extra (performance only) */
  int64_t pair_sims;          /* simulations summed over the timed pair launches (a large batch runs as two half batches) */
  int64_t box_flips;          /* triclinic box flips applied during straining runs (fix deform, default flip yes) */
  /* force_field "reax": the matrix sweep of the charge equilibration (k_rx_qeq_sweep), the HBM-bound kernel of that path */
  int64_t rx_sweep_launches;  /* timed launches */
  double rx_sweep_ms;         /* sum of their HIP-event durations */
  double rx_sweep_entries;    /* stored matrix entries those launches passed over (per replica: entries of its rows x sweeps it took
                               * part in); algorithmic bytes = (8 value + rx_sweep_col_bytes) per entry + 84 per row */
  double rx_sweep_rows;       /* rows likewise */
  int64_t rx_sweep_col_bytes; /* bytes of a stored column index beside the 8-byte value: 0 (replicas of up to 65 536 atoms: it rides in the value's word) or 4 */
  /* Launches on different streams may be in flight together (a batch runs as two half batches): the time during which AT LEAST ONE of the
   * timed launches ran -- the union of their HIP-event intervals on the device's common clock.  Equal to the sums above when nothing overlaps. */
  double pair_union_ms;
  double rx_sweep_union_ms;
  int64_t rx_sweep_symmetric; /* 1: the timed sweeps ran in the symmetric form (each pair of the matrix stored once, in its owner's row: rx_sweep_entries
                               * counts stored entries, half of the full rows'); 0: full rows */
  int64_t row_cell_builds;    /* row potentials: the neighbour-list builds (part of neigh_builds) of replicas whose rows are built through cells */
} scema_md_profile;
int scema_md_get_profile(scema_md_engine *e, scema_md_profile *out, int32_t reset);

/* The library reads its environment through ONE table of declared switches (scema_amd/csrc/md_env.h, engine/engine_core.cpp:
 * performance A/B switches with measured defaults, test hooks, diagnostics; the reference has no counterpart -- its knobs are the
 * LAMMPS scripts).  This returns the declared switches that are set in the calling process's environment as "NAME=value" lines,
 * and their number: a reported run shows an empty list (bench.py: config.env_overrides). */
int scema_md_env_overrides(char *buf, int cap);

/* Calibration of the box a measurement ran on (no counterpart in the reference; measurement aid of bench.py): independent FP64 FMA
 * chains on every SIMD of the device, no memory traffic, ~0.1 s (a warm-up launch, then the best of three).  The boxes of a pool differ by several per cent under the pair
 * kernel's full-chip FP64 load; this figure (74-75 TFLOP/s on an MI355X at its sustained clock, 78.6 on the data sheet) lets
 * throughput values of different boxes be normalised.  Needs a HIP device; returns SCEMA_MD_ERR_DEVICE without one. */
int scema_md_box_fma_tflops(int32_t device, double *tflops);

/* The k-space set-up a run would use for this box, as a pure host function (no GPU, no engine): LAMMPS' initial g_ewald estimate
 * from the accuracy asked for (what `kspace_style ewald` keeps), and for kspace_style 1 the PPPM grid and the adjusted g_ewald by
 * PPPM::set_grid_global / adjust_gewald as restated in engine/engine_kspace.cpp (in.set.lammps:36 `kspace_style pppm 0.0001`).
 * grid = 0 0 0 for the Ewald sum or an uncharged system.  For checks against an independent restatement of those rules
 * (tests/test_oracle_pppm.py) and against LAMMPS' own log line "G vector ... grid = ..." (tools/export_lammps_case.py --run). */
int scema_md_kspace_setup(const scema_md_params *p, const double *box /* 9: lo[3] hi[3] xy xz yz */, double qsqsum /* sum q_i^2, e^2 */,
                          int32_t natoms, double *g_initial, double *g_ewald, int32_t *grid /* 3 */);

#ifdef __cplusplus
}
#endif
#endif
