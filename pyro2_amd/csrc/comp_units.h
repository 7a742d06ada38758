// What the compressible units export to comp_api.hip: THE list -- a new host function of a unit is one
// line here.  Included inside namespace pyro::PYRO_NS, like fused_common.h (no include guard): by the
// six defining units, so that a definition whose signature drifts leaves the declared one undefined
// and the link fails (build.py: --no-undefined), and by comp_api.hip once per namespace.  What each
// function does stands at its definition.

// ---- both builds define these (comp_api.hip: PYRO_BUILD) ----
int comp_dt(pyrohip_state *, const pyrohip_comp_params *, double, double *);                    // compressible.hip
int comp_cfl_min_device(pyrohip_state *, const pyrohip_comp_params *, const double **);         // compressible.hip
int comp_step_staged(pyrohip_state *, const pyrohip_comp_params *, double);                     // compressible.hip
int comp_fill_frame_user(pyrohip_state *, const pyrohip_comp_params *, const StepScalars *, double *);   // compressible.hip
int comp_fill_frame_user_parts(const pyrohip_state *);                                          // compressible.hip
int comp_sponge_run(pyrohip_state *, const pyrohip_comp_params *, const StepScalars *, double *);   // compressible.hip
int comp_sponge_run_parts(const pyrohip_state *);                                               // compressible.hip
int comp_dt_sph(pyrohip_state *, const pyrohip_comp_params *, double, double *);                // compressible.hip
int comp_cfl_min_device_sph(pyrohip_state *, const pyrohip_comp_params *, const double **);     // compressible.hip
int comp_step_sph(pyrohip_state *, const pyrohip_comp_params *, double);                        // compressible.hip
int comp_rk_rhs(pyrohip_state *, const pyrohip_comp_params *, pyrohip_state *, int);            // compressible.hip
int comp_step_fused(pyrohip_state *, const pyrohip_comp_params *, double);                      // comp_fused.hip
int comp_step_fused_ex(pyrohip_state *, const pyrohip_comp_params *, double, const StepScalars *,
                       const double **);                                                        // comp_fused.hip
int comp_fused_tiles(const pyrohip_state *);                                                    // comp_fused.hip
int comp_step_fused_batch(pyrohip_state *, const pyrohip_comp_params *, const BatchMember *, int, int);   // comp_fused.hip
int comp_step_fused_sph(pyrohip_state *, const pyrohip_comp_params *, double);                  // comp_fused.hip
int comp_step_fused_sph_ex(pyrohip_state *, const pyrohip_comp_params *, double, const StepScalars *,
                           const double **);                                                    // comp_fused.hip
int comp_step_wave(pyrohip_state *, const pyrohip_comp_params *, double);                       // comp_wave.hip
int comp_step_wave_ex(pyrohip_state *, const pyrohip_comp_params *, double, const StepScalars *,
                      const double **);                                                         // comp_wave.hip
int comp_rk_rhs_wave(pyrohip_state *, const pyrohip_comp_params *, pyrohip_state *, int);       // comp_wave.hip
int comp_rk_step_wave(pyrohip_state *, const pyrohip_comp_params *, pyrohip_state *, int, const double *,
                      const double *, double, const StepScalars *, const double **);            // comp_wave.hip
int comp_step_wave_sph(pyrohip_state *, const pyrohip_comp_params *, double);                   // comp_sph_wave.hip
int comp_step_wave_sph_ex(pyrohip_state *, const pyrohip_comp_params *, double, const StepScalars *,
                          const double **);                                                     // comp_sph_wave.hip
int comp_fv4_rhs(pyrohip_state *, const pyrohip_comp_params *, pyrohip_state *, int);           // comp_fv4.hip
int comp_fv4_rhs_run(pyrohip_state *, const pyrohip_comp_params *, pyrohip_state *, int, const StepScalars *,
                     int *);                                                                    // comp_fv4.hip
int comp_rk_step_tile(pyrohip_state *, const pyrohip_comp_params *, pyrohip_state *, int, const double *,
                      const double *, double, const StepScalars *, const double **);            // comp_rk_tile.hip

// ---- the bit-faithful build alone exports these: never contracted, or no arithmetic at all
// (comp_api.hip: exact::).  Most are defined under #if !PYRO_FAST; of the ones a contracted unit
// compiles as well, nothing calls that copy.  A unit declares them where PYRO_FAST says so;
// comp_api.hip names the build it declares with PYRO_UNITS_FAST. ----
#ifndef PYRO_UNITS_FAST
#define PYRO_UNITS_FAST PYRO_FAST
#endif
#if !PYRO_UNITS_FAST
int comp_sponge(pyrohip_state *, const pyrohip_comp_params *, double);                          // compressible.hip
int comp_source_correct(pyrohip_state *, const pyrohip_comp_params *, double);                  // compressible.hip
int comp_stage_dump(pyrohip_state *, int, double *);                                            // compressible.hip
int comp_rk_dt(pyrohip_state *, const pyrohip_comp_params *, double, double *);                 // compressible.hip
int comp_rk_cfl_min_device(pyrohip_state *, const pyrohip_comp_params *, const double **);      // compressible.hip
int comp_wave_geometry(int, int, int, int, int, int *);                                         // comp_wave.hip
int comp_wave_plan(int, int, int, int, int, int, int *);                                        // comp_wave.hip
int sph_wave_geometry(int, int, int, int, int, int *);                                          // comp_sph_wave.hip
void rk_tile_geometry(int, int, int *, int *, int *);                                           // comp_rk_tile.hip
int state_from_centers(pyrohip_state *, int, double, double, double *);                         // comp_fv4.hip
int comp_sdc_update(pyrohip_state *, const pyrohip_state *, const pyrohip_state *, int, int, const int *,
                    const double *, double);                                                    // comp_fv4.hip
int fv4_stage_start(pyrohip_state *, const pyrohip_state *, const pyrohip_state *, const double *, int,
                    const StepScalars *);                                                       // comp_fv4.hip
int fv4_sdc_node(pyrohip_state *, const pyrohip_state *, const pyrohip_state *, int, int, const int *,
                 const double *, const StepScalars *, const int *);                             // comp_fv4.hip
int fv4_final_parts(const Geom &);                                                              // comp_fv4.hip
int fv4_final(pyrohip_state *, const pyrohip_state *, const pyrohip_state *, const double *, int,
              const pyrohip_comp_params *, const StepScalars *, double *);                      // comp_fv4.hip
int fv4_copy_frame(pyrohip_state *, const double *);                                            // comp_fv4.hip
#endif
#undef PYRO_UNITS_FAST
