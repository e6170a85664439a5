/*
 * SolRStub.h - flat extern "C" facade over the singleton engine.
 *
 * Same names, argument order and return conventions as the reference's
 * solr/SolRStub.h:36-135 (0 / -1 ints, doubles converted to floats, no C++
 * exceptions across the boundary) for every call that feeds or runs the
 * rendering path, including the scene-file loaders (SolR_LoadMolecule,
 * SolR_LoadOBJModel, SolR_SaveToFile, SolR_LoadFromFile) and the texture-file
 * loader (SolR_LoadTextureFromFile) and the screenshot (SolR_GenerateScreenshot:
 * a JPEG file, byte for byte the one the reference's encoder writes for the
 * same frame).  Not provided (out of scope): the three
 * OpenCL-device queries and the Kinect call.
 *
 * SolRx_* are extensions used by the test-suite and bench.py: engine
 * selection, deterministic timestamps/randoms, access to the flattened arrays
 * and to the float framebuffer.
 */
#pragma once

#include "../../include/solr_hip.h"
#include "../../include/solr_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------- Scene (SolRStub.h:44-60) ---------- */
int SolR_SetSceneInfo(int width, int height, int graphicsLevel, int nbRayIterations, double transparentColor,
                      double viewDistance, double shadowIntensity, double eyeSeparation, double bgColorR,
                      double bgColorG, double bgColorB, double bgColorA, int renderBoxes, int pathTracingIteration,
                      int maxPathTracingIterations, int frameBufferType, int timestamp, int atmosphericEffect,
                      int cameraType, int doubleSidedTriangles, int extendedGeometry, int advancedIllumination,
                      int skyboxSize, int skyboxMaterialId, double geometryEpsilon, double rayEpsilon);
int SolR_SetPostProcessingInfo(int type, double param1, double param2, int param3);
int SolR_SetDraftMode(int draft);
int SolR_InitializeKernel(bool activeLogging, int platform, int device);
int SolR_FinalizeKernel();
int SolR_ResetKernel();

/* ---------- Camera (SolRStub.h:65-66) ---------- */
void SolR_SetCamera(double eye_x, double eye_y, double eye_z, double dir_x, double dir_y, double dir_z,
                    double angle_x, double angle_y, double angle_z);

/* ---------- Rendering (SolRStub.h:69) ---------- */
int SolR_RunKernel(double timer, BitmapBuffer *image);

/* ---------- Primitives (SolRStub.h:72-103) ---------- */
int SolR_AddPrimitive(int type, int movable);
int SolR_SetPrimitive(int index, double p0_x, double p0_y, double p0_z, double p1_x, double p1_y, double p1_z,
                      double p2_x, double p2_y, double p2_z, double size_x, double size_y, double size_z,
                      int materialId);
int SolR_GetPrimitive(int index, double *p0_x, double *p0_y, double *p0_z, double *p1_x, double *p1_y, double *p1_z,
                      double *p2_x, double *p2_y, double *p2_z, double *size_x, double *size_y, double *size_z,
                      int *materialId);
int SolR_GetPrimitiveAt(int x, int y);
int SolR_GetPrimitiveCenter(int index, double *x, double *y, double *z);
int SolR_RotatePrimitives(int fromBoxId, int toBoxId, double rx, double ry, double rz, double ax, double ay,
                          double az);
int SolR_SetPrimitiveMaterial(int index, int materialId);
int SolR_GetPrimitiveMaterial(int index);
int SolR_SetPrimitiveNormals(int index, double n0_x, double n0_y, double n0_z, double n1_x, double n1_y, double n1_z,
                             double n2_x, double n2_y, double n2_z);
int SolR_SetPrimitiveTextureCoordinates(int index, double t0_x, double t0_y, double t1_x, double t1_y, double t2_x,
                                        double t2_y);

/* ---------- Materials (SolRStub.h:106-125) ---------- */
int SolR_AddMaterial();
int SolR_SetMaterial(int index, double color_r, double color_g, double color_b, double noise, double reflection,
                     double refraction, int procedural, int wireframe, int wireframeDepth, double transparency,
                     double opacity, int diffuseTextureId, int normalTextureId, int bumpTextureId,
                     int specularTextureId, int reflectionTextureId, int transparencyTextureId,
                     int ambientOcclusionTextureId, double specValue, double specPower, double specCoef,
                     double innerIllumination, double illuminationDiffusion, double illuminationPropagation,
                     int fastTransparency);

/* ---------- Read-back of materials and textures (SolRStub.h:114-122,133) ---------- */
/* the reference's `type &out` parameters are pointers here: the same ABI.  -1 (outputs untouched) for an
 * index beyond the active materials */
int SolR_GetMaterial(int index, double *color_r, double *color_g, double *color_b, double *noise, double *reflection,
                     double *refraction, int *procedural, int *wireframe, int *wireframeDepth, double *transparency,
                     double *opacity, int *diffuseTextureId, int *normalTextureId, int *bumpTextureId,
                     int *specularTextureId, int *reflectionTextureId, int *transparencyTextureId,
                     int *ambientOcclusionTextureId, double *specValue, double *specPower, double *specCoef,
                     double *innerIllumination, double *illuminationDiffusion, double *illuminationPropagation,
                     int *fastTransparency);
/* the texture's pixels with the first and third channel swapped (SolRStub.cpp:351-373); 0 = done, 1 = no
 * such texture */
int SolR_GetTexture(int index, BitmapBuffer *image);
/* accepted for compatibility: the reference's SolR_RotatePrimitive is an empty TODO (SolRStub.cpp:232-240),
 * and there is nothing to recompile at run time - the kernels are built ahead of time for gfx950 */
int SolR_RotatePrimitive(int index, double rx, double ry, double rz, double ax, double ay, double az);
int SolR_RecompileKernels(char *filename);

/* ---------- Scene files (SolRStub.h:145-146) ---------- */
/* .irt scene dumps, host/FileMarshaller.h; both return the number of active (flattened) primitives,
 * which is what the reference returns: 0 until the next SolR_CompactBoxes */
/* Molecules from PDB files, host/PDBReader.h (SolRStub.h:137-138): geometryType 0 atoms, 1 fixed-size atoms,
 * 2 sticks, 3 atoms and sticks, 4 iso-surface, 5 backbone; atomMaterialType 0 by element, 1 by chain,
 * 2 by residue.  Materials 0..118 are overwritten with the element colours. */
int SolR_LoadMolecule(char *filename, int geometryType, double defaultAtomSize, double defaultStickSize,
                      int atomMaterialType, double scale);
/* Wavefront OBJ + MTL, host/OBJReader.h (SolRStub.h:141-143; the reference passes `double &height`, the
 * same ABI).  The model's materials take the ids materialId, materialId + 1, ... in the order of the MTL
 * file; *height receives -(scaled model height) / 2. */
int SolR_LoadOBJModel(char *filename, int materialId, int autoScale, double scale, int autoCenter, double *height);
/* SWC neuron morphology, host/SWCReader.h.  The reference has the reader (solr/io/SWCReader.cpp, used by
 * its SwcScene) but no stub entry for it; this one passes loadMorphologyFromFile's arguments through and
 * returns the number of samples read. */
int SolRx_LoadSWCMorphology(const char *filename, double px, double py, double pz, double sx, double sy, double sz,
                            double sw, int materialId);
/* ... and the samples the reader kept of the morphology loaded last (SWCReader::getMorphologies, what the reference's
 * SwcScene walks along), by ascending id: coordinates and radius as scaled by the load, primitiveId the primitive the reader
 * stored with the sample (the root's sphere, the cylinder of a sample that has children below the root's; 0 where it made
 * none).  Writes the first min(count, capacity) records and returns the count; samples == NULL: the count alone */
typedef struct SolrSwcSample
{
    int id, branch;
    float x, y, z, radius;
    int parent, primitiveId;
} SolrSwcSample;
int SolRx_GetMorphologies(SolrSwcSample *samples, int capacity);
int SolR_SaveToFile(char *filename);
int SolR_LoadFromFile(char *filename, double scale);

/* ---------- Boxes / lights (SolRStub.h:128-131) ---------- */
int SolR_CompactBoxes(bool update);
int SolR_GetLight(int index);

/* ---------- Textures (SolRStub.h:134-138).  The reference's SolR_SetTexture
 * is an empty TODO (SolRStub.cpp:357-366); this one takes the pixels. */
int SolR_SetTexture(int index, const unsigned char *pixels, int width, int height, int depth, int textureType);
int SolR_GetTextureSize(int index, int *width, int *height, int *depth);
int SolR_GetNbTextures(int *nbTextures);
/* SolRStub.h:130.  A .bmp, .tga or .jpg file into slot `index` (GPUKernel::loadTextureFromFile).  Returns the
 * reference's bool (SolRStub.cpp:313-317): 1 = loaded, 0 = not - NOT the 0 / -1 of its neighbours */
int SolR_LoadTextureFromFile(int index, char *filename);
/* extension: the TextureType the loader derived from the file's name, -1 for a slot out of range */
int SolRx_GetTextureType(int index);

/* ---------- Screenshots (SolRStub.h:62) ---------- */
/* `quality` passes of path tracing at width x height (at most 1920 x 1080), the last image as a JPEG file of JPEG
 * quality 85 with 2x2 chroma (the reference encoder's defaults); always 0, as in the reference */
int SolR_GenerateScreenshot(char *filename, int width, int height, int quality);
/* the screenshot's encoder on the caller's width * height * 3 bytes: JPEG quality 1..100, luma sampling 1x1, 2x1 or
 * 2x2; turned / swapRedBlue read the pixels as a screenshot reads a frame (include/solr_hip.h, SolrJpegSource) */
int SolRx_EncodeJpeg(const char *filename, const unsigned char *pixels, int width, int height, int jpegQuality,
                     int lumaH, int lumaV, int turned, int swapRedBlue);
/* the two halves of the encoder and its division, for the tests (SolRStub.cpp) */
int SolRx_JpegCoefficients(const unsigned char *pixels, int width, int height, int jpegQuality, int lumaH, int lumaV,
                           int turned, int swapRedBlue, short *coefficients, long nbBlocks);
int SolRx_JpegFromCoefficients(const char *filename, const short *coefficients, long nbBlocks, int width, int height,
                               int jpegQuality, int lumaH, int lumaV);
int SolRx_JpegQuantise(int q, int first, int count, int negative, short *out);
/* one frame as SolR_RunKernel renders it, as a JPEG file in the caller's `file` of `capacity` bytes (*nbBytes its size):
 * JPEG quality 1..100, luma sampling 1x1, 2x1 or 2x2, read as a screenshot reads a frame.  With the HIP engine the frame
 * is coded on the device and only the file's bytes come to the host; SolRx_GetBitmap() is not refreshed.  0; -1 for
 * arguments out of range, a failed frame (*nbBytes = 0), or a file that does not fit (*nbBytes = what it takes) */
int SolRx_RenderJpeg(double timer, int jpegQuality, int lumaH, int lumaV, unsigned char *file, long capacity,
                     long *nbBytes);
/* the file of SolRx_JpegFromCoefficients in memory, its entropy-coded segment by the engine's entropy stage
 * (csrc/jpeg_entropy.h: kernels with the HIP engine, loops without a device); same returns */
int SolRx_JpegFileFromCoefficients(const short *coefficients, long nbBlocks, int width, int height, int jpegQuality,
                                   int lumaH, int lumaV, unsigned char *file, long capacity, long *nbBytes);
/* SolRx_EncodeJpeg, SolRx_RenderJpeg and SolRx_JpegFileFromCoefficients with optimised Huffman tables: the file of the
 * reference encoder's two-pass mode - four tables built for the picture's own symbols (csrc/jpeg_entropy.h, optimiseTable;
 * with the HIP engine counted and built on the device) in its DHT segments - which decodes to the same pixels and is
 * smaller.  Same arguments and returns */
int SolRx_EncodeJpegOptimised(const char *filename, const unsigned char *pixels, int width, int height, int jpegQuality,
                              int lumaH, int lumaV, int turned, int swapRedBlue);
int SolRx_RenderJpegOptimised(double timer, int jpegQuality, int lumaH, int lumaV, unsigned char *file, long capacity,
                              long *nbBytes);
int SolRx_JpegFileFromCoefficientsOptimised(const short *coefficients, long nbBlocks, int width, int height,
                                            int jpegQuality, int lumaH, int lumaV, unsigned char *file, long capacity,
                                            long *nbBytes);
/* the host's table builder: counts[0 ... len - 1] (len 1 ... 256) to bits[16] and values[len]; returns the number of
 * values, or -1 for arguments out of range.  SolRx_JpegCensus: the symbols of nbBlocks blocks with lumaBlocks (1, 2 or 4)
 * luma blocks per MCU, added up in counts[536] - DC luma 12, DC chroma 12, AC luma 256, AC chroma 256; 0, or -1 when a
 * block is outside the domain (nothing written).  SolRx_JpegEncodeTwoPass: the one-pass bit-buffer writer
 * (JpegWriter::encode) in its optimised mode, to a file - next to SolRx_JpegFromCoefficients */
int SolRx_JpegOptimiseTable(const unsigned int *counts, int len, unsigned char *bits, unsigned char *values);
int SolRx_JpegCensus(const short *coefficients, long nbBlocks, int lumaBlocks, unsigned int *counts);
int SolRx_JpegFromCoefficientsOptimised(const char *filename, const short *coefficients, long nbBlocks, int width,
                                        int height, int jpegQuality, int lumaH, int lumaV);
/* JPEG frames in flight: SolRx_RenderJpegBegin renders the next frame - on the next flight with SolRx_SetFramesInFlight(n),
 * nothing flushed - and submits it for delivery as a JPEG file (optimised != 0: with tables built for the frame); a ticket
 * >= 0, or -1.  SolRx_RenderJpegEnd waits for that frame alone and hands over its file: 0, or -1 as SolRx_RenderJpeg - a
 * capacity too small leaves the size in *nbBytes and the ticket good: the second call renders nothing.  A ticket may be
 * collected any number of times until three more have been handed out; a stale or never-issued one gives -1 with
 * *nbBytes = 0 and SolRx_RenderJpegTicketError's text set (0: the last SolRx_RenderJpegEnd had nothing to say).  With the
 * HIP engine nothing waits for the device between the two calls; where it declines (no device, strips, several devices)
 * the frame is rendered and encoded at once and the file kept under the ticket.  May be mixed with SolRx_FlushFrames,
 * SolR_RunKernel and SolRx_RenderJpeg */
int SolRx_RenderJpegBegin(double timer, int jpegQuality, int lumaH, int lumaV, int optimised);
int SolRx_RenderJpegEnd(int ticket, unsigned char *file, long capacity, long *nbBytes);
int SolRx_RenderJpegTicketError(char *buf, int len);
/* for the tests: pixels parked under such a ticket; the plan of the resident entropy pipeline (SolRStub.cpp) */
int SolRx_JpegParkPixels(const unsigned char *pixels, int width, int height, int jpegQuality, int lumaH, int lumaV,
                         int swapRedBlue, int optimised);
void SolRx_JpegEntropyPlan(unsigned long long totalBits, int flag, long nbBlocks, unsigned long long out[9]);
void SolRx_JpegEntropyStreamSizes(unsigned long long totalBits, unsigned long long out[3]);
/* csrc/jpeg_entropy.h for the tests (SolRStub.cpp) */
void SolRx_JpegEntropyGranularity(int out[2]);
void SolRx_JpegEntropyPrefix(const unsigned int *lengths, long n, unsigned long long *offsets);
int SolRx_JpegBlockBits(const short *block, int previousDc, int chroma);
/* GPUKernel::resetFrame: the current frame's primitives, boxes and lamps dropped, materials and textures kept - what a
 * scene that makes its geometry anew every frame begins a frame with */
int SolRx_ResetFrame();
/* the iso-surface of a field of metaballs appended to the scene as triangles of material materialId
 * (GPUKernel::addMetaballs; grid, balls and the order of the triangles: include/solr_hip.h).  With the HIP engine the field
 * and the cubes run on the device.  The number of triangles added, -1 on error (nothing is added then) */
int SolRx_AddMetaballs(const SolrIsoGrid *grid, const float *balls, int nbBalls, int materialId);
/* for the tests: the two halves through the current engine (solr_hip_iso_field / solr_hip_iso_surface or the loops over
 * csrc/iso_surface.h; same arguments and results), and the engine's table of cases: count[256] triangles per case,
 * edges[256][15] their cube edges */
int SolRx_IsoField(const SolrIsoGrid *grid, const float *balls, int nbBalls, float *field);
int SolRx_IsoSurface(const SolrIsoGrid *grid, const float *field, SolrIsoTriangle *triangles, int capacity);
int SolRx_IsoCaseTable(unsigned char *count, unsigned char *edges);
/* which atoms of a molecule are joined by a stick, through the current engine (GPUKernel::stickPairsOf: solr_hip_stick_pairs
 * or the loops over csrc/stick_pairs.h; arguments and results as include/solr_hip.h gives them for solr_hip_stick_pairs: the
 * number of pairs there are, start whole, the first min(total, capacity) partners).  -1 for arguments out of range */
long long SolRx_StickPairs(const float *atoms, const unsigned char *backbone, int n, float reachPlain, float reachBackbone,
                           long long *start, int *partners, long long capacity);
/* searches served since the library was loaded: out[0] by a device, out[1] by the loops on the CPU */
void SolRx_StickSearches(long long out[2]);
/* the number of atoms from which the HIP engine searches on the device (GPUKernel::setStickDeviceFrom; below it the loops
 * on the CPU are quicker than the fixed cost of a call; 0: always on the device).  Returns the value before */
int SolRx_SetStickDeviceFrom(int n);
/* for the tests: the threshold on the squared sum that stands for `reach` (csrc/stick_pairs.h squaredReach) */
float SolRx_StickSquaredReach(float reach);
/* seconds SolR_LoadMolecule spent last in its three steps: file to map, search for the sticks, primitives added */
void SolRx_MoleculeLoadTimes(double out[3]);

/* ---------- Extensions ---------- */
/* "hip" (default) or "host-only"; destroys the current singleton */
int SolRx_SelectEngine(const char *name);
/* seed >= 0: keep SceneInfo.timestamp and fill the random buffer from a seeded
 * LCG; seed < 0: reference behaviour (rand()/time(0)) */
int SolRx_SetDeterministic(long seed);
/* 1: compactBoxes(true) always builds the box tree on the host; 0 (default): on the device when the engine
 * offers it (include/solr_hip.h solr_hip_build_tree) - the same tree either way.  Also SOLR_HOST_BUILD=1 */
int SolRx_HostBuild(int hostOnly);
/* pending engine error: 0 = none; copies the text into buf when non-null */
int SolRx_LastError(char *buf, int len);
/* render_begin + render_end without copying the bitmap */
int SolRx_Render(double timer);
/* frames in flight through SolR_RunKernel / SolRx_Render (GPUKernel::setFramesInFlight, 1 ... 4; 1 = the reference's
 * protocol): a call delivers the image of the frame n - 1 calls back while the newer ones render;
 * SolRx_FlushFrames waits for all of them; SolRx_GetBitmap is the image delivered last, without a copy */
int SolRx_SetFramesInFlight(int n);
int SolRx_GetFramesInFlight();
int SolRx_FlushFrames(void);
/* the frame shared out over n devices of this process (occupancyParameters.x of the boundary, include/solr_hip.h);
 * returns the number in use, or -1.  With frames in flight the ids behind SolR_GetPrimitiveAt are the newest
 * frame's, up to n - 1 frames ahead of the image on show. */
int SolRx_SetGpuCount(int n);
const BitmapBuffer *SolRx_GetBitmap(void);
/* flattened arrays of the current frame (owned by the engine, valid until
 * the next compactBoxes / material change) */
int SolRx_GetBoxes(const BoundingBox **boxes, int *nbBoxes);
int SolRx_GetPrimitives(const Primitive **primitives, int *nbPrimitives);
int SolRx_GetLights(const LightInformation **lights, int *nbLights, int *nbLamps);
int SolRx_GetMaterials(const Material **materials, int *nbMaterials);
int SolRx_GetRandoms(const float **randoms, int *nbRandoms);
int SolRx_GetTextureAtlas(const unsigned char **atlas, long *nbBytes);
int SolRx_GetPrimitiveIds(const PrimitiveXYIdBuffer **ids, int *nbPixels);
int SolRx_GetSceneInfo(SceneInfo *sceneInfo, PostProcessingInfo *postProcessingInfo, float eye[3], float dir[3],
                       float angles[4]);
int SolRx_GetTreeDepth();
/* rotations applied on the device that the host scene store has not replayed yet; SolRx_SyncHost replays them */
/* key frames (GPUKernel::setNbFrames / setFrame / morphPrimitives; the reference's scenes call them directly) */
int SolRx_SetNbFrames(int nbFrames);
int SolRx_GetNbFrames();
int SolRx_SetFrame(int frame);
int SolRx_MorphPrimitives();
/* the current frame - one between the key frames, e.g. as SolRx_MorphPrimitives made it - blended anew at any finite weight
 * (0: the first key frame, 1: the last; beyond: extrapolated), its tree kept in shape and refitted
 * (GPUKernel::morphFrame).  0 = done, -1 = refused, nothing changed.  SolRx_PendingMorph: 1 while such a morph was
 * applied on the device and the host scene store has not replayed it yet (SolRx_SyncHost replays it) */
int SolRx_MorphFrame(double weight);
/* the same with any two frames as the keys: the current frame - a stage that is neither of them - set to
 * frameA + weight * (frameB - frameA), material, texture coordinates and movable flag those of frameA
 * (GPUKernel::morphBetween).  An animation of K key frames of one mesh plays through it: SolRx_MorphBetween(k, k + 1, t).
 * 0 = done and flattened, -1 = refused, nothing changed; SolRx_PendingMorph as above */
int SolRx_MorphBetween(int frameA, int frameB, double weight);
/* whether rotations move the primitive, set after SolR_SetPrimitive (which makes it movable); a morph takes the first key's */
int SolRx_SetPrimitiveIsMovable(int index, int movable);
int SolRx_PendingMorph();
int SolRx_PendingRotations();
/* the other rigid moves of a scene (the reference's stub has no call for either): GPUKernel::translatePrimitives, and
 * GPUKernel::setPrimitiveCenter - the viewer's lamp drag -, each followed by compactBoxes(false) as the reference's
 * applications follow them.  With the HIP engine and an unchanged resident scene a translation, and the centre of a
 * primitive that is a lamp, are applied on the device.  SolRx_PendingMoves: rotations, translations and lamp moves applied
 * there that the host scene store has not replayed yet (SolRx_PendingRotations: the rotations among them) */
int SolRx_TranslatePrimitives(double x, double y, double z);
int SolRx_SetPrimitiveCenter(int index, double x, double y, double z);
/* a batch of primitives of the store set anew (GPUKernel::setPrimitives: per record setPrimitive and, by flag,
 * setPrimitiveNormals and setPrimitiveTextureCoordinates; then the box updates) + compactBoxes(false).  With the HIP engine
 * and an unchanged resident scene the batch is applied on the device and counts among SolRx_PendingMoves.  0 = done, -1 =
 * an index is not in the store: nothing changed.  SolRx_SizeofPrimitiveEdit: the record's size, for bindings */
int SolRx_SetPrimitives(const SolrPrimitiveEdit *edits, int n);
/* a batch of primitives of the store given another material (GPUKernel::setPrimitiveMaterials: per record
 * setPrimitiveMaterial, of several records for one index the last one wins) + compactBoxes(false): what the reference's
 * SwcScene does per frame, a viewer to highlight a picked primitive, a molecule scene to recolour atoms.  With the HIP engine
 * and an unchanged resident scene the batch is applied on the device and counts among SolRx_PendingMoves;
 * SolR_GetPrimitiveMaterial answers what is pending.  0 = done, -1 = an index is not in the store: nothing changed */
int SolRx_SetPrimitiveMaterials(const int *indices, const int *materialIds, int n);
int SolRx_SizeofPrimitiveEdit();
int SolRx_PendingMoves();
/* the frame bank (GPUKernel::setFrameBank): with `bytes` > 0 a frame that SolRx_SetFrame leaves stays on the engine - up to
 * that many bytes of device memory in all - and comes back with no flatten and no upload when it is entered again; 0, the
 * default, is off.  SolRx_ParkedFrames: frames set aside now; SolRx_FrameSwitches: switches served from the bank;
 * SolRx_SceneUploads: uploads of the scene, both since the kernel was made */
int SolRx_SetFrameBank(unsigned long long bytes);
int SolRx_ParkedFrames();
int SolRx_FrameSwitches();
int SolRx_SceneUploads();
/* material edits on the resident scene (GPUKernel::setMaterialEdits): with `on` != 0 a material set between two frames
 * (SolR_SetMaterial and its kin) is followed by the HIP engine in place - the changed records of its table, the tags and
 * colour keys of the primitives that have the material - where it can, and the table is uploaded as ever where it declines
 * (the first frame after an upload of the scene, a table that has grown, a primitive the walks would have to treat as another
 * kind, see include/solr_hip.h solr_hip_edit_materials); 0, the default, is off: the upload as ever.  The lamps' light records
 * keep the colours of the last flatten either way.  SolRx_MaterialEdits: edits followed in place since the kernel was made */
int SolRx_SetMaterialEdits(int on);
int SolRx_MaterialEdits();
int SolRx_SyncHost();
int SolRx_GetMovable(const unsigned char **flags, int *nbPrimitives);
/* float framebuffer of the last frame, W*H records */
int SolRx_GetPostProcessingBuffer(PostProcessingBuffer *buffer);
/* camera with an explicit angles.w (SolR_SetCamera forces 6400) */
void SolRx_SetCameraW(double eye_x, double eye_y, double eye_z, double dir_x, double dir_y, double dir_z,
                      double angle_x, double angle_y, double angle_z, double angle_w);
int SolRx_AddRectangle(double x, double y, double z, double w, double h, double d, int materialId);
int SolRx_SetSceneInfoExtras(int gradientBackground, int draftMode);

#ifdef __cplusplus
}
#endif
